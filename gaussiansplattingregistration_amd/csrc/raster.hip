// raster.hip -- forward tile rasteriser of a splat model for one pinhole camera (gsr_raster_*) and the image metrics of the
// evaluation stage (gsr_image_metrics).  DESIGN.md section 14.
//
// Render: k_raster_preprocess (projection, conic, radius, SH colour, tile count) -> exclusive scan of the 64-bit counts -> ONE
// host read-back of the intersection total -> k_raster_emit (keys (tile id << 32 | depth bits), values = splat index) -> radix
// sort limited to the bits in use (stable: equal depths keep ascending splat index) -> k_raster_ranges -> k_raster_blend, one
// 256-thread work-group per 16 x 16 tile.  No float atomics: every pixel sums its splats front to back in the sorted order, so
// an image is the same bits from run to run.  The two counters (visible splats, non-empty tiles) are integer atomics.
//
// The semantics restate the published 3DGS / gsplat forward pass (EWA projection with the clamped perspective Jacobian, 0.3 px
// dilation, 3-sigma integer radius, alpha clamp 0.999, 1/255 skip, transmittance stop at 1e-4); gsplat itself is not available on
// ROCm, so parity with it is unpinned.  tests/raster_model.py is the executable restatement the kernels are held to.
//
// gsr_raster_render_aux is the same pipeline with another blend, k_raster_blend_aux: coverage 1 - T, expected
// depth sum(z w) / alpha and, per splat, the largest blending weight w = alpha T it reaches on any pixel (an integer atomicMax on
// the float's bits: still no float atomics).  tests/raster_aux_model.py restates it.
//
// gsr_raster_backward is the backward pass of that render: the same pipeline up to the tile ranges, then
// k_raster_blend_bwd (one record of nine floats per splat-tile intersection, folded over the tile in a fixed tree) and k_raster_splat_bwd
// (every splat adds its records in a fixed order and runs the projection backwards).  No float atomics either; tests/raster_grad_model.py
// restates it.
#include <math.h>
#include <string.h>

#include <rocprim/rocprim.hpp>

#include "gsr_common.h"
#include "gsr_oneshot.h"

using namespace gsr;

namespace {

constexpr int TILE = 16;
constexpr int BLEND_THREADS = TILE * TILE;          // four waves
constexpr int SPLAT_WORDS = 9;                      // mean2d xy, conic A B C, opacity, r g b: 36 bytes

struct RasterCam {
    float R[9], t[3], cam[3];                       // world -> camera rotation (row-major), translation; camera position in the world
    float fx, fy, cx, cy;
    float lim_xp, lim_xn, lim_yp, lim_yn;           // the frustum in x/z, y/z widened by 0.3 tan(fov/2) on each side
    float near_z, far_z, eps2d, radius_clip;
    int32_t W, H, tiles_x, tiles_y, degree, K;
};

// SH colour in the basis 3DGS evaluates; rest[k*3 + c], k = 0 .. K-1 (coefficient-major).  d is a unit vector.
__device__ __forceinline__ void sh_colour(int degree, const float* __restrict__ dc, const float* __restrict__ rest, float x, float y, float z, float* rgb) {
    const float C0 = 0.28209479177387814f, C1 = 0.4886025119029199f;
    const float C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f, -1.0925484305920792f, 0.5462742152960396f};
    const float C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f, 0.3731763325901154f, -0.4570457994644658f, 1.445305721320277f,
                         -0.5900435899266435f};
    float b[15];
    int nb = 0;
    if (degree > 0) {
        b[0] = -C1 * y; b[1] = C1 * z; b[2] = -C1 * x;
        nb = 3;
        if (degree > 1) {
            const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            b[3] = C2[0] * xy; b[4] = C2[1] * yz; b[5] = C2[2] * (2.0f * zz - xx - yy); b[6] = C2[3] * xz; b[7] = C2[4] * (xx - yy);
            nb = 8;
            if (degree > 2) {
                b[8] = C3[0] * y * (3.0f * xx - yy);
                b[9] = C3[1] * xy * z;
                b[10] = C3[2] * y * (4.0f * zz - xx - yy);
                b[11] = C3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy);
                b[12] = C3[4] * x * (4.0f * zz - xx - yy);
                b[13] = C3[5] * z * (xx - yy);
                b[14] = C3[6] * x * (xx - 3.0f * yy);
                nb = 15;
            }
        }
    }
    for (int c = 0; c < 3; ++c) {
        float v = C0 * dc[c];
        for (int k = 0; k < nb; ++k) v = v + b[k] * rest[3 * k + c];
        rgb[c] = fmaxf(v + 0.5f, 0.0f);
    }
}

// One thread per splat: everything the blend needs (splat[i*9 ..]), its depth, its tile box and the number of tiles it touches
// (0 = culled).  counters[0] += visible splats (one integer atomic per wave).
__global__ __launch_bounds__(256) void k_raster_preprocess(int64_t n, RasterCam cam, const float* __restrict__ xyz, const float* __restrict__ cov6,
                                                           const float* __restrict__ raw_opacity, const float* __restrict__ dc,
                                                           const float* __restrict__ sh_rest, float* __restrict__ splat, float* __restrict__ depth,
                                                           ushort4* __restrict__ rect, int64_t* __restrict__ counts, unsigned long long* __restrict__ counters) {
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < n; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = base + threadIdx.x;
        int64_t touched = 0;
        if (i < n) {
            const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
            const float* R = cam.R;
            const float px = ((R[0] * x + R[1] * y) + R[2] * z) + cam.t[0];
            const float py = ((R[3] * x + R[4] * y) + R[5] * z) + cam.t[1];
            const float pz = ((R[6] * x + R[7] * y) + R[8] * z) + cam.t[2];
            bool ok = pz >= cam.near_z && pz <= cam.far_z;
            float a = 0.f, b = 0.f, c = 0.f, det = 0.f, mx = 0.f, my = 0.f, rad = 0.f;
            if (ok) {
                const float* s = cov6 + 6 * i;
                const float S[3][3] = {{s[0], s[1], s[2]}, {s[1], s[3], s[4]}, {s[2], s[4], s[5]}};
                float M[3][3], Sc[3][3];
                for (int r = 0; r < 3; ++r)
                    for (int q = 0; q < 3; ++q) M[r][q] = (R[3 * r] * S[0][q] + R[3 * r + 1] * S[1][q]) + R[3 * r + 2] * S[2][q];
                for (int r = 0; r < 3; ++r)
                    for (int q = r; q < 3; ++q) Sc[r][q] = Sc[q][r] = (M[r][0] * R[3 * q] + M[r][1] * R[3 * q + 1]) + M[r][2] * R[3 * q + 2];
                const float rz = 1.0f / pz;
                const float tx = pz * fminf(cam.lim_xp, fmaxf(-cam.lim_xn, px * rz));
                const float ty = pz * fminf(cam.lim_yp, fmaxf(-cam.lim_yn, py * rz));
                const float rz2 = rz * rz;
                const float j00 = cam.fx * rz, j02 = -(cam.fx * tx) * rz2, j11 = cam.fy * rz, j12 = -(cam.fy * ty) * rz2;
                const float v00 = Sc[0][0] * j00 + Sc[0][2] * j02, v01 = Sc[1][0] * j00 + Sc[1][2] * j02, v02 = Sc[2][0] * j00 + Sc[2][2] * j02;
                const float v11 = Sc[1][1] * j11 + Sc[1][2] * j12, v12 = Sc[2][1] * j11 + Sc[2][2] * j12;
                a = (j00 * v00 + j02 * v02) + cam.eps2d;
                b = j11 * v01 + j12 * v02;
                c = (j11 * v11 + j12 * v12) + cam.eps2d;
                det = a * c - b * b;
                ok = det > 0.0f;
                mx = (cam.fx * px) * rz + cam.cx;
                my = (cam.fy * py) * rz + cam.cy;
            }
            if (ok) {
                const float bm = 0.5f * (a + c);
                rad = ceilf(3.0f * sqrtf(bm + sqrtf(fmaxf(0.01f, bm * bm - det))));
                ok = rad > cam.radius_clip && !(mx + rad <= 0.0f || mx - rad >= (float)cam.W || my + rad <= 0.0f || my - rad >= (float)cam.H);
            }
            if (ok) {
                const float inv = 1.0f / (float)TILE;
                // clamped as floats: a far-off mean or a huge radius must not reach the conversion to int
                const float fx_t = (float)cam.tiles_x, fy_t = (float)cam.tiles_y;
                const int x0 = (int)fminf(fmaxf(floorf((mx - rad) * inv), 0.0f), fx_t), x1 = (int)fminf(fmaxf(ceilf((mx + rad) * inv), 0.0f), fx_t);
                const int y0 = (int)fminf(fmaxf(floorf((my - rad) * inv), 0.0f), fy_t), y1 = (int)fminf(fmaxf(ceilf((my + rad) * inv), 0.0f), fy_t);
                touched = (int64_t)(x1 - x0) * (int64_t)(y1 - y0);
                ok = touched > 0;
                if (ok) {
                    float dx = x - cam.cam[0], dy = y - cam.cam[1], dz = z - cam.cam[2];
                    const float il = 1.0f / sqrtf((dx * dx + dy * dy) + dz * dz);
                    dx *= il; dy *= il; dz *= il;
                    float rgb[3];
                    sh_colour(cam.degree, dc + 3 * i, sh_rest ? sh_rest + 3 * (int64_t)cam.K * i : nullptr, dx, dy, dz, rgb);
                    float* o = splat + SPLAT_WORDS * i;
                    o[0] = mx; o[1] = my;
                    o[2] = c / det; o[3] = -b / det; o[4] = a / det;
                    o[5] = 1.0f / (1.0f + expf(-raw_opacity[i]));
                    o[6] = rgb[0]; o[7] = rgb[1]; o[8] = rgb[2];
                    depth[i] = pz;
                    rect[i] = make_ushort4((unsigned short)x0, (unsigned short)y0, (unsigned short)x1, (unsigned short)y1);
                } else touched = 0;
            }
            counts[i] = touched;
        }
        const unsigned long long vis = __ballot(touched > 0);
        if ((threadIdx.x & 63) == 0 && vis) atomicAdd(&counters[0], (unsigned long long)__popcll(vis));
    }
}

// counts[n] is the slot behind the last splat: scanned with the rest, offsets[n] is the intersection total
__global__ void k_raster_emit(int64_t n, int32_t tiles_x, const float* __restrict__ depth, const ushort4* __restrict__ rect,
                              const int64_t* __restrict__ counts, const int64_t* __restrict__ offsets, int64_t total, uint64_t* __restrict__ keys,
                              uint32_t* __restrict__ vals) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (counts[i] <= 0) continue;
        const ushort4 r = rect[i];
        const uint64_t d = (uint64_t)__float_as_uint(depth[i]);
        int64_t o = offsets[i];
        for (int ty = r.y; ty < r.w; ++ty)
            for (int tx = r.x; tx < r.z; ++tx, ++o)
                if (o < total) {                                       // cannot fail: the scan of these very counts sized the buffers
                    keys[o] = ((uint64_t)(uint32_t)(ty * tiles_x + tx) << 32) | d;
                    vals[o] = (uint32_t)i;
                }
    }
}

// ranges[2 t], ranges[2 t + 1]: first and one-past-last sorted position of tile t (zeroed before: an empty tile is [0, 0))
__global__ void k_raster_ranges(int64_t total, int32_t n_tiles, const uint64_t* __restrict__ keys, int64_t* __restrict__ ranges,
                                unsigned long long* __restrict__ counters) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t t = (uint32_t)(keys[i] >> 32);
        if (t >= (uint32_t)n_tiles) continue;
        if (i == 0 || (uint32_t)(keys[i - 1] >> 32) != t) { ranges[2 * (int64_t)t] = i; atomicAdd(&counters[2], 1ull); }
        if (i == total - 1 || (uint32_t)(keys[i + 1] >> 32) != t) ranges[2 * (int64_t)t + 1] = i + 1;
    }
}

// One work-group per tile, one thread per pixel (wave w holds rows 4 w .. 4 w + 3).  Batches of 256 sorted splats are staged in
// LDS (stride 9 words: conflict-free writes, broadcast reads); a wave whose ballot shows no live pixel skips the batch, and the
// group leaves when all four say so.
__global__ __launch_bounds__(BLEND_THREADS) void k_raster_blend(int32_t W, int32_t H, int32_t tiles_x, float bg0, float bg1, float bg2, int64_t n,
                                                                const int64_t* __restrict__ ranges, const uint32_t* __restrict__ vals,
                                                                const float* __restrict__ splat, float* __restrict__ image) {
    __shared__ float s_splat[BLEND_THREADS * SPLAT_WORDS];
    __shared__ int s_alive[BLEND_THREADS / 64];
    const int t = threadIdx.x, wave = t >> 6;
    const int tile = blockIdx.y * tiles_x + blockIdx.x;
    const int ix = blockIdx.x * TILE + (t & (TILE - 1)), iy = blockIdx.y * TILE + (t >> 4);
    const bool inside = ix < W && iy < H;
    const float px = (float)ix + 0.5f, py = (float)iy + 0.5f;
    const int64_t first = ranges[2 * (int64_t)tile], last = ranges[2 * (int64_t)tile + 1];
    float T = 1.0f, r = 0.0f, g = 0.0f, b = 0.0f;
    bool done = !inside;
    for (int64_t base = first; base < last; base += BLEND_THREADS) {
        const bool wave_alive = __ballot(!done) != 0ull;
        if ((t & 63) == 0) s_alive[wave] = wave_alive ? 1 : 0;
        const int64_t pos = base + t;
        if (pos < last) {
            const uint32_t id = vals[pos];
            if ((int64_t)id < n) {
                const float* src = splat + (int64_t)SPLAT_WORDS * id;
#pragma unroll
                for (int k = 0; k < SPLAT_WORDS; ++k) s_splat[SPLAT_WORDS * t + k] = src[k];
            } else {                                               // never: an index the emit kernel did not write
#pragma unroll
                for (int k = 0; k < SPLAT_WORDS; ++k) s_splat[SPLAT_WORDS * t + k] = 0.0f;
            }
        }
        __syncthreads();
        if (!(s_alive[0] | s_alive[1] | s_alive[2] | s_alive[3])) break;
        if (wave_alive) {
            const int m = (int)((last - base) < (int64_t)BLEND_THREADS ? (last - base) : (int64_t)BLEND_THREADS);
            for (int j = 0; j < m && !done; ++j) {
                const float* s = s_splat + SPLAT_WORDS * j;
                const float dx = s[0] - px, dy = s[1] - py;
                const float sigma = 0.5f * (s[2] * dx * dx + s[4] * dy * dy) + s[3] * dx * dy;
                if (sigma < 0.0f) continue;
                const float alpha = fminf(0.999f, s[5] * expf(-sigma));
                if (alpha < 1.0f / 255.0f) continue;
                const float Tn = T * (1.0f - alpha);
                if (Tn <= 1e-4f) { done = true; break; }
                const float vis = alpha * T;
                r = r + s[6] * vis; g = g + s[7] * vis; b = b + s[8] * vis;
                T = Tn;
            }
        }
        __syncthreads();
    }
    if (inside) {
        float* o = image + 3 * ((int64_t)iy * W + ix);
        o[0] = r + T * bg0; o[1] = g + T * bg1; o[2] = b + T * bg2;
    }
}

// The largest value of a wave, in every lane's view of lane 63: four row_shr steps leave each row of 16 lanes its inclusive maxima,
// row_bcast15 and row_bcast31 carry the row ends across.  A lane without a source keeps `old` = 0, the identity of a maximum of
// unsigned values.  All 64 lanes must be active.
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    uint32_t o;
    o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false); v = v > o ? v : o;      // row_shr:1
    o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false); v = v > o ? v : o;      // row_shr:2
    o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false); v = v > o ? v : o;      // row_shr:4
    o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false); v = v > o ? v : o;      // row_shr:8
    o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false); v = v > o ? v : o;      // row_bcast15 into rows 1, 3
    o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false); v = v > o ? v : o;      // row_bcast31 into rows 2, 3
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// The blend with the auxiliary outputs of DESIGN.md 22: the same pixel loop in the same float32 order (a requested image is the bits
// k_raster_blend writes), plus D = sum z w per pixel (s_z: the tenth staged word, kept out of the stride-9 record) and, with CONTRIB,
// the largest w = alpha T of every staged splat: s_contrib[j] belongs to the thread that staged splat j, which zeroes it, lets the
// waves raise it between the barriers and sends it to contribution[id] with one integer atomicMax after the closing barrier
// (non-negative floats order as their bit patterns: no float atomics, no dependence on the order).  With CONTRIB the j loop is
// wave-uniform -- it runs while any lane is live, finished lanes offer 0 -- so that the wave's maximum is taken by DPP steps and one
// lane raises the slot.  image, depth, alpha: each NULL or written (wave-uniform tests).
template <bool CONTRIB>
__global__ __launch_bounds__(BLEND_THREADS) void k_raster_blend_aux(int32_t W, int32_t H, int32_t tiles_x, float bg0, float bg1, float bg2, int64_t n,
                                                                    const int64_t* __restrict__ ranges, const uint32_t* __restrict__ vals,
                                                                    const float* __restrict__ splat, const float* __restrict__ zs, float* __restrict__ image,
                                                                    float* __restrict__ depth, float* __restrict__ alpha_out, uint32_t* __restrict__ contribution) {
    __shared__ float s_splat[BLEND_THREADS * SPLAT_WORDS];
    __shared__ float s_z[BLEND_THREADS];
    __shared__ uint32_t s_contrib[CONTRIB ? BLEND_THREADS : 1];
    __shared__ int s_alive[BLEND_THREADS / 64];
    const int t = threadIdx.x, wave = t >> 6;
    const int tile = blockIdx.y * tiles_x + blockIdx.x;
    const int ix = blockIdx.x * TILE + (t & (TILE - 1)), iy = blockIdx.y * TILE + (t >> 4);
    const bool inside = ix < W && iy < H;
    const float px = (float)ix + 0.5f, py = (float)iy + 0.5f;
    const int64_t first = ranges[2 * (int64_t)tile], last = ranges[2 * (int64_t)tile + 1];
    float T = 1.0f, r = 0.0f, g = 0.0f, b = 0.0f, D = 0.0f;
    bool done = !inside;
    for (int64_t base = first; base < last; base += BLEND_THREADS) {
        const bool wave_alive = __ballot(!done) != 0ull;
        if ((t & 63) == 0) s_alive[wave] = wave_alive ? 1 : 0;
        const int64_t pos = base + t;
        int64_t my_id = -1;                                        // the splat this thread staged, if it may be reported
        if (pos < last) {
            const uint32_t id = vals[pos];
            if ((int64_t)id < n) {
                const float* src = splat + (int64_t)SPLAT_WORDS * id;
#pragma unroll
                for (int k = 0; k < SPLAT_WORDS; ++k) s_splat[SPLAT_WORDS * t + k] = src[k];
                s_z[t] = zs[id];
                my_id = (int64_t)id;
            } else {                                               // never: an index the emit kernel did not write
#pragma unroll
                for (int k = 0; k < SPLAT_WORDS; ++k) s_splat[SPLAT_WORDS * t + k] = 0.0f;
                s_z[t] = 0.0f;
            }
        }
        if (CONTRIB) s_contrib[t] = 0u;
        __syncthreads();
        if (!(s_alive[0] | s_alive[1] | s_alive[2] | s_alive[3])) break;       // (every slot is still zero: nothing to send)
        if (wave_alive) {
            const int m = (int)((last - base) < (int64_t)BLEND_THREADS ? (last - base) : (int64_t)BLEND_THREADS);
            if (CONTRIB) {
                for (int j = 0; j < m; ++j) {
                    if (__ballot(!done) == 0ull) break;
                    float w = 0.0f;
                    if (!done) {
                        const float* s = s_splat + SPLAT_WORDS * j;
                        const float dx = s[0] - px, dy = s[1] - py;
                        const float sigma = 0.5f * (s[2] * dx * dx + s[4] * dy * dy) + s[3] * dx * dy;
                        if (!(sigma < 0.0f)) {
                            const float alpha = fminf(0.999f, s[5] * expf(-sigma));
                            if (!(alpha < 1.0f / 255.0f)) {
                                const float Tn = T * (1.0f - alpha);
                                if (Tn <= 1e-4f) done = true;
                                else {
                                    const float vis = alpha * T;
                                    r = r + s[6] * vis; g = g + s[7] * vis; b = b + s[8] * vis;
                                    D = D + s_z[j] * vis;
                                    T = Tn;
                                    w = vis;
                                }
                            }
                        }
                    }
                    const uint32_t top = wave_max_u32(__float_as_uint(w));       // w >= 0: its bits order as it does
                    if (top != 0u && (t & 63) == 0) atomicMax(&s_contrib[j], top);
                }
            } else {
                for (int j = 0; j < m && !done; ++j) {
                    const float* s = s_splat + SPLAT_WORDS * j;
                    const float dx = s[0] - px, dy = s[1] - py;
                    const float sigma = 0.5f * (s[2] * dx * dx + s[4] * dy * dy) + s[3] * dx * dy;
                    if (sigma < 0.0f) continue;
                    const float alpha = fminf(0.999f, s[5] * expf(-sigma));
                    if (alpha < 1.0f / 255.0f) continue;
                    const float Tn = T * (1.0f - alpha);
                    if (Tn <= 1e-4f) { done = true; break; }
                    const float vis = alpha * T;
                    r = r + s[6] * vis; g = g + s[7] * vis; b = b + s[8] * vis;
                    D = D + s_z[j] * vis;
                    T = Tn;
                }
            }
        }
        __syncthreads();
        if (CONTRIB && my_id >= 0) {
            const uint32_t top = s_contrib[t];
            if (top != 0u) atomicMax(contribution + my_id, top);
        }
    }
    if (inside) {
        const int64_t p = (int64_t)iy * W + ix;
        if (image) {
            float* o = image + 3 * p;
            o[0] = r + T * bg0; o[1] = g + T * bg1; o[2] = b + T * bg2;
        }
        const float a = 1.0f - T;
        if (alpha_out) alpha_out[p] = a;
        if (depth) depth[p] = D / fmaxf(a, 1e-10f);
    }
}

// ---- backward pass (gsr_raster_backward) -------------------------------------------------------------------
// The sum of a wave, valid in lane 63, as the tree of adjacent pairs: the four row_shr steps leave lane 15 of each row
// ((x15 + x14) + (x13 + x12)) + ... , row_bcast15 adds row 0 to row 1 and row 2 to row 3, row_bcast31 adds lane 31 to lane 63.  A lane
// without a source adds `old` = +0.0.  All 64 lanes must be active.  One row is one pixel row of the tile, a wave four of them.
__device__ __forceinline__ float wave_sum_f32(float v) {
    float o;
    o = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xf, 0xf, false)); v = v + o;      // row_shr:1
    o = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x112, 0xf, 0xf, false)); v = v + o;      // row_shr:2
    o = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x114, 0xf, 0xf, false)); v = v + o;      // row_shr:4
    o = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x118, 0xf, 0xf, false)); v = v + o;      // row_shr:8
    o = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x142, 0xa, 0xf, false)); v = v + o;      // row_bcast15 into rows 1, 3
    o = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x143, 0xc, 0xf, false)); v = v + o;      // row_bcast31 into rows 2, 3
    return v;
}

// One work-group per tile, one thread per pixel, as the forward.  First the forward walk (the loop of k_raster_blend without the
// colours): every pixel keeps T_end and the sorted position of its last counted splat.  Positions behind the last one any pixel of
// the tile counted get zero records at once.  Then the sorted splats are walked back to front, in the forward's batches of 256, the
// last batch first: T <- T / (1 - alpha) recovers the transmittance in front of a splat, `acc` carries (sum of the w c behind it +
// T_end bg) . G_C.  Every lane offers nine terms per staged splat (mean2d xy, conic A B C, opacity, r g b; 0 when the pixel did not
// count it), a wave folds them with wave_sum_f32 and lane 63 leaves them in s_part (a wave with no contributing lane leaves +0.0,
// a wave with no counted splat in the batch is left out: x + 0.0 = x); after the batch thread j adds the four waves in order and
// writes the nine floats of the splat it staged (stride 9 words over the lanes: odd, conflict-free) to that intersection's record, at
// the slot the emission gave it.  Every record of the tile's range is written, no float atomics.  grad_image, grad_alpha: each NULL (zeros) or read.
__global__ __launch_bounds__(BLEND_THREADS) void k_raster_blend_bwd(int32_t W, int32_t H, int32_t tiles_x, float bg0, float bg1, float bg2, int64_t n,
                                                                    const int64_t* __restrict__ ranges, const uint32_t* __restrict__ vals,
                                                                    const float* __restrict__ splat, const ushort4* __restrict__ rect,
                                                                    const int64_t* __restrict__ offsets, int64_t total,
                                                                    const float* __restrict__ grad_image, const float* __restrict__ grad_alpha,
                                                                    float* __restrict__ rec) {
    __shared__ float s_splat[BLEND_THREADS * SPLAT_WORDS];
    __shared__ float s_part[(BLEND_THREADS / 64) * BLEND_THREADS * SPLAT_WORDS];
    __shared__ int s_alive[BLEND_THREADS / 64];
    __shared__ int s_count;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int tile = blockIdx.y * tiles_x + blockIdx.x;
    const int ix = blockIdx.x * TILE + (t & (TILE - 1)), iy = blockIdx.y * TILE + (t >> 4);
    const bool inside = ix < W && iy < H;
    const float px = (float)ix + 0.5f, py = (float)iy + 0.5f;
    const int64_t first = ranges[2 * (int64_t)tile], last = ranges[2 * (int64_t)tile + 1];
    if (first >= last) return;
    if (t == 0) s_count = 0;
    float T = 1.0f;
    int last_cnt = -1;                                             // offset from `first` of the last splat this pixel counted
    bool done = !inside;
    for (int64_t base = first; base < last; base += BLEND_THREADS) {
        const bool wave_alive = __ballot(!done) != 0ull;
        if (lane == 0) s_alive[wave] = wave_alive ? 1 : 0;
        const int64_t pos = base + t;
        if (pos < last) {
            const uint32_t id = vals[pos];
            const bool known = (int64_t)id < n;
            const float* src = splat + (int64_t)SPLAT_WORDS * (known ? id : 0u);
#pragma unroll
            for (int k = 0; k < 6; ++k) s_splat[SPLAT_WORDS * t + k] = known ? src[k] : 0.0f;
        }
        __syncthreads();
        if (!(s_alive[0] | s_alive[1] | s_alive[2] | s_alive[3])) break;
        if (wave_alive) {
            const int m = (int)((last - base) < (int64_t)BLEND_THREADS ? (last - base) : (int64_t)BLEND_THREADS);
            for (int j = 0; j < m && !done; ++j) {
                const float* s = s_splat + SPLAT_WORDS * j;
                const float dx = s[0] - px, dy = s[1] - py;
                const float sigma = 0.5f * (s[2] * dx * dx + s[4] * dy * dy) + s[3] * dx * dy;
                if (sigma < 0.0f) continue;
                const float alpha = fminf(0.999f, s[5] * expf(-sigma));
                if (alpha < 1.0f / 255.0f) continue;
                const float Tn = T * (1.0f - alpha);
                if (Tn <= 1e-4f) { done = true; break; }
                T = Tn;
                last_cnt = (int)(base - first) + j;
            }
        }
        __syncthreads();
    }
    if (last_cnt >= 0) atomicMax(&s_count, last_cnt + 1);         // an integer maximum in LDS
    __syncthreads();
    const int count = s_count;                                     // positions first .. first + count - 1 are walked back
    // where the record of a sorted position goes: the slot k_raster_emit gave this (splat, tile) pair, offsets[id] + the tile's row-major
    // index in the splat's box -- the inverse of the sort, computed instead of stored.  -1: never (an index the emit kernel did not write)
    const int tile_x = blockIdx.x, tile_y = blockIdx.y;
    auto slot_of = [&](uint32_t id) -> int64_t {
        if ((int64_t)id >= n) return -1;
        const ushort4 r = rect[id];
        if (tile_x < r.x || tile_x >= r.z || tile_y < r.y || tile_y >= r.w) return -1;
        const int64_t slot = offsets[id] + (int64_t)(tile_y - r.y) * (r.z - r.x) + (tile_x - r.x);
        return slot < total ? slot : -1;
    };
    for (int64_t pos = first + count + t; pos < last; pos += BLEND_THREADS) {
        const int64_t slot = slot_of(vals[pos]);
        if (slot >= 0) {
#pragma unroll
            for (int k = 0; k < SPLAT_WORDS; ++k) rec[SPLAT_WORDS * slot + k] = 0.0f;
        }
    }

    float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f, gA = 0.0f;
    if (inside) {
        const int64_t p = (int64_t)iy * W + ix;
        if (grad_image) { g0 = grad_image[3 * p]; g1 = grad_image[3 * p + 1]; g2 = grad_image[3 * p + 2]; }
        if (grad_alpha) gA = grad_alpha[p];
    }
    const float T_end = T;
    const float tga = T_end * gA;
    float acc = T_end * ((bg0 * g0 + bg1 * g1) + bg2 * g2);
    for (int b = (count - 1) / BLEND_THREADS; b >= 0 && count > 0; --b) {
        const int off0 = b * BLEND_THREADS;
        const int m = count - off0 < BLEND_THREADS ? count - off0 : BLEND_THREADS;
        const bool wave_live = __ballot(last_cnt >= off0) != 0ull;
        if (lane == 0) s_alive[wave] = wave_live ? 1 : 0;
        int64_t my_slot = -1;
        if (t < m) {
            const uint32_t id = vals[first + off0 + t];
            const bool known = (int64_t)id < n;
            const float* src = splat + (int64_t)SPLAT_WORDS * (known ? id : 0u);
#pragma unroll
            for (int k = 0; k < SPLAT_WORDS; ++k) s_splat[SPLAT_WORDS * t + k] = known ? src[k] : 0.0f;
            my_slot = slot_of(id);
        }
        __syncthreads();
        const int live0 = s_alive[0], live1 = s_alive[1], live2 = s_alive[2], live3 = s_alive[3];
        if (wave_live) {
            for (int j = m - 1; j >= 0; --j) {
                float v[SPLAT_WORDS];
#pragma unroll
                for (int k = 0; k < SPLAT_WORDS; ++k) v[k] = 0.0f;
                bool counted = false;
                if (off0 + j <= last_cnt) {
                    const float* s = s_splat + SPLAT_WORDS * j;
                    const float dx = s[0] - px, dy = s[1] - py;
                    const float sigma = 0.5f * (s[2] * dx * dx + s[4] * dy * dy) + s[3] * dx * dy;
                    if (!(sigma < 0.0f)) {
                        const float e = expf(-sigma);
                        const float araw = s[5] * e;
                        const float alpha = fminf(0.999f, araw);
                        if (!(alpha < 1.0f / 255.0f)) {
                            counted = true;
                            const float om = 1.0f - alpha;
                            T = T / om;
                            const float w = alpha * T;
                            const float cg = (s[6] * g0 + s[7] * g1) + s[8] * g2;
                            v[6] = w * g0; v[7] = w * g1; v[8] = w * g2;
                            const float dalpha = T * cg - (acc - tga) / om;
                            acc = acc + w * cg;
                            if (!(araw > 0.999f)) {                            // not clamped: sigma and the opacity take part
                                v[5] = e * dalpha;
                                const float gs = -(alpha * dalpha);
                                v[0] = gs * (s[2] * dx + s[3] * dy);
                                v[1] = gs * (s[4] * dy + s[3] * dx);
                                v[2] = gs * (0.5f * (dx * dx));
                                v[3] = gs * (dx * dy);
                                v[4] = gs * (0.5f * (dy * dy));
                            }
                        }
                    }
                }
                float* part = s_part + SPLAT_WORDS * (wave * BLEND_THREADS + j);
                if (__ballot(counted) != 0ull) {
#pragma unroll
                    for (int k = 0; k < SPLAT_WORDS; ++k) v[k] = wave_sum_f32(v[k]);
                    if (lane == 63) {
#pragma unroll
                        for (int k = 0; k < SPLAT_WORDS; ++k) part[k] = v[k];
                    }
                } else if (lane < SPLAT_WORDS) part[lane] = 0.0f;
            }
        }
        __syncthreads();
        if (my_slot >= 0) {
            float* o = rec + (int64_t)SPLAT_WORDS * my_slot;
#pragma unroll
            for (int k = 0; k < SPLAT_WORDS; ++k) {
                float sum = live0 ? s_part[SPLAT_WORDS * t + k] : 0.0f;
                sum = sum + (live1 ? s_part[SPLAT_WORDS * (BLEND_THREADS + t) + k] : 0.0f);
                sum = sum + (live2 ? s_part[SPLAT_WORDS * (2 * BLEND_THREADS + t) + k] : 0.0f);
                sum = sum + (live3 ? s_part[SPLAT_WORDS * (3 * BLEND_THREADS + t) + k] : 0.0f);
                o[k] = sum;
            }
        }
    }
}

// The SH colour backwards: gv = dL/d(colour before the + 0.5 and the clamp) per channel (0 on a clamped channel).  g_dc, g_rest (each NULL
// or written: coefficients beyond the degree get 0) and gd += dL/d(unit direction) through the basis.
__device__ __forceinline__ void sh_colour_bwd(int degree, int K, const float* __restrict__ rest, float x, float y, float z, const float* gv,
                                              float* __restrict__ g_dc, float* __restrict__ g_rest, float* gd) {
    const float C0 = 0.28209479177387814f, C1 = 0.4886025119029199f;
    const float C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f, -1.0925484305920792f, 0.5462742152960396f};
    const float C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f, 0.3731763325901154f, -0.4570457994644658f, 1.445305721320277f,
                         -0.5900435899266435f};
    if (g_dc) { g_dc[0] = C0 * gv[0]; g_dc[1] = C0 * gv[1]; g_dc[2] = C0 * gv[2]; }
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
    // coefficient k with basis value bk and its derivatives along x, y, z
    auto term = [&](int k, float bk, float ddx, float ddy, float ddz) {
        const float* r = rest + 3 * k;
        const float gb = (r[0] * gv[0] + r[1] * gv[1]) + r[2] * gv[2];
        gx = gx + gb * ddx; gy = gy + gb * ddy; gz = gz + gb * ddz;
        if (g_rest) { g_rest[3 * k] = bk * gv[0]; g_rest[3 * k + 1] = bk * gv[1]; g_rest[3 * k + 2] = bk * gv[2]; }
    };
    int nb = 0;
    if (degree > 0) {
        term(0, -C1 * y, 0.0f, -C1, 0.0f);
        term(1, C1 * z, 0.0f, 0.0f, C1);
        term(2, -C1 * x, -C1, 0.0f, 0.0f);
        nb = 3;
        if (degree > 1) {
            const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            term(3, C2[0] * xy, C2[0] * y, C2[0] * x, 0.0f);
            term(4, C2[1] * yz, 0.0f, C2[1] * z, C2[1] * y);
            term(5, C2[2] * (2.0f * zz - xx - yy), C2[2] * (-2.0f * x), C2[2] * (-2.0f * y), C2[2] * (4.0f * z));
            term(6, C2[3] * xz, C2[3] * z, 0.0f, C2[3] * x);
            term(7, C2[4] * (xx - yy), C2[4] * (2.0f * x), C2[4] * (-2.0f * y), 0.0f);
            nb = 8;
            if (degree > 2) {
                term(8, C3[0] * y * (3.0f * xx - yy), C3[0] * (6.0f * xy), C3[0] * (3.0f * xx - 3.0f * yy), 0.0f);
                term(9, C3[1] * xy * z, C3[1] * yz, C3[1] * xz, C3[1] * xy);
                term(10, C3[2] * y * (4.0f * zz - xx - yy), C3[2] * (-2.0f * xy), C3[2] * (4.0f * zz - xx - 3.0f * yy), C3[2] * (8.0f * yz));
                term(11, C3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy), C3[3] * (-6.0f * xz), C3[3] * (-6.0f * yz), C3[3] * (6.0f * zz - 3.0f * xx - 3.0f * yy));
                term(12, C3[4] * x * (4.0f * zz - xx - yy), C3[4] * (4.0f * zz - 3.0f * xx - yy), C3[4] * (-2.0f * xy), C3[4] * (8.0f * xz));
                term(13, C3[5] * z * (xx - yy), C3[5] * (2.0f * xz), C3[5] * (-2.0f * yz), C3[5] * (xx - yy));
                term(14, C3[6] * x * (xx - 3.0f * yy), C3[6] * (3.0f * xx - 3.0f * yy), C3[6] * (-6.0f * xy), 0.0f);
                nb = 15;
            }
        }
    }
    if (g_rest)
        for (int k = 3 * nb; k < 3 * K; ++k) g_rest[k] = 0.0f;
    gd[0] = gx; gd[1] = gy; gd[2] = gz;
}

// One thread per splat.  A culled splat (counts = 0) writes +0.0 to every output.  A visible one adds the records of the tiles of its rect
// in the order k_raster_emit wrote them (ty outer, tx inner) -- k_raster_blend_bwd left them at the emission's slots, offsets[i] onwards,
// so they are read in a row, without a search -- nine float32 accumulators.  Then the chain of k_raster_preprocess backwards, every forward
// value recomputed with the forward's expressions (opacity and colour are read from the staged splat): conic -> (a, b, c) ->
// (Sigma_c -> cov6; J -> p_c), mean2d -> p_c, p_c -> xyz, sigmoid -> raw opacity, colour -> dc, sh_rest and, through the unit direction,
// xyz.  Outputs: each NULL or overwritten.
__global__ __launch_bounds__(256) void k_raster_splat_bwd(int64_t n, RasterCam cam, const float* __restrict__ xyz, const float* __restrict__ cov6,
                                                          const float* __restrict__ sh_rest, const float* __restrict__ splat,
                                                          const int64_t* __restrict__ counts, const int64_t* __restrict__ offsets,
                                                          const float* __restrict__ rec, float* __restrict__ g_xyz, float* __restrict__ g_cov6,
                                                          float* __restrict__ g_raw_opacity, float* __restrict__ g_dc, float* __restrict__ g_sh_rest) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float* o_rest = g_sh_rest ? g_sh_rest + 3 * (int64_t)cam.K * i : nullptr;
        if (counts[i] <= 0) {
            if (g_xyz) { g_xyz[3 * i] = 0.0f; g_xyz[3 * i + 1] = 0.0f; g_xyz[3 * i + 2] = 0.0f; }
            if (g_cov6)
                for (int k = 0; k < 6; ++k) g_cov6[6 * i + k] = 0.0f;
            if (g_raw_opacity) g_raw_opacity[i] = 0.0f;
            if (g_dc) { g_dc[3 * i] = 0.0f; g_dc[3 * i + 1] = 0.0f; g_dc[3 * i + 2] = 0.0f; }
            if (o_rest)
                for (int k = 0; k < 3 * cam.K; ++k) o_rest[k] = 0.0f;
            continue;
        }
        float g[SPLAT_WORDS];
#pragma unroll
        for (int k = 0; k < SPLAT_WORDS; ++k) g[k] = 0.0f;
        const float* r = rec + (int64_t)SPLAT_WORDS * offsets[i];
        for (int64_t tile = 0; tile < counts[i]; ++tile, r += SPLAT_WORDS) {
#pragma unroll
            for (int k = 0; k < SPLAT_WORDS; ++k) g[k] = g[k] + r[k];
        }
        // the forward values, as k_raster_preprocess forms them
        const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        const float* R = cam.R;
        const float px = ((R[0] * x + R[1] * y) + R[2] * z) + cam.t[0];
        const float py = ((R[3] * x + R[4] * y) + R[5] * z) + cam.t[1];
        const float pz = ((R[6] * x + R[7] * y) + R[8] * z) + cam.t[2];
        const float* s = cov6 + 6 * i;
        const float S[3][3] = {{s[0], s[1], s[2]}, {s[1], s[3], s[4]}, {s[2], s[4], s[5]}};
        float M[3][3], Sc[3][3];
        for (int r = 0; r < 3; ++r)
            for (int q = 0; q < 3; ++q) M[r][q] = (R[3 * r] * S[0][q] + R[3 * r + 1] * S[1][q]) + R[3 * r + 2] * S[2][q];
        for (int r = 0; r < 3; ++r)
            for (int q = r; q < 3; ++q) Sc[r][q] = Sc[q][r] = (M[r][0] * R[3 * q] + M[r][1] * R[3 * q + 1]) + M[r][2] * R[3 * q + 2];
        const float rz = 1.0f / pz;
        const float ux = px * rz, uy = py * rz;
        const float tx = pz * fminf(cam.lim_xp, fmaxf(-cam.lim_xn, ux));
        const float ty = pz * fminf(cam.lim_yp, fmaxf(-cam.lim_yn, uy));
        // on the clamped branch t = z lim: nothing to x (or y), lim to z
        const bool clx = ux > cam.lim_xp || ux < -cam.lim_xn, cly = uy > cam.lim_yp || uy < -cam.lim_yn;
        const float limx = ux > cam.lim_xp ? cam.lim_xp : -cam.lim_xn, limy = uy > cam.lim_yp ? cam.lim_yp : -cam.lim_yn;
        const float rz2 = rz * rz;
        const float j00 = cam.fx * rz, j02 = -(cam.fx * tx) * rz2, j11 = cam.fy * rz, j12 = -(cam.fy * ty) * rz2;
        const float v00 = Sc[0][0] * j00 + Sc[0][2] * j02, v01 = Sc[1][0] * j00 + Sc[1][2] * j02, v02 = Sc[2][0] * j00 + Sc[2][2] * j02;
        const float v11 = Sc[1][1] * j11 + Sc[1][2] * j12, v12 = Sc[2][1] * j11 + Sc[2][2] * j12;
        const float a = (j00 * v00 + j02 * v02) + cam.eps2d;
        const float b = j11 * v01 + j12 * v02;
        const float c = (j11 * v11 + j12 * v12) + cam.eps2d;
        const float det = a * c - b * b;
        // conic (c, -b, a) / det -> a, b, c
        const float di = 1.0f / det, di2 = di * di;
        const float ga = di2 * (((b * c) * g[3] - (c * c) * g[2]) - (b * b) * g[4]);
        const float gc = di2 * (((a * b) * g[3] - (b * b) * g[2]) - (a * a) * g[4]);
        const float gb = di2 * (((2.0f * (b * c)) * g[2] - (a * c + b * b) * g[3]) + (2.0f * (a * b)) * g[4]);
        // (a, b, c) = J Sigma_c J^T -> Sigma_c (each off-diagonal entry once for its two positions) -> cov6 = R^T G R
        if (g_cov6) {
            const float s00 = ga * (j00 * j00), s01 = gb * (j00 * j11), s02 = ga * (2.0f * (j00 * j02)) + gb * (j00 * j12);
            const float s11 = gc * (j11 * j11), s12 = gb * (j02 * j11) + gc * (2.0f * (j11 * j12));
            const float s22 = (ga * (j02 * j02) + gb * (j02 * j12)) + gc * (j12 * j12);
            const float G[3][3] = {{s00, 0.5f * s01, 0.5f * s02}, {0.5f * s01, s11, 0.5f * s12}, {0.5f * s02, 0.5f * s12, s22}};
            float N[3][3], Gw[3][3];
            for (int r = 0; r < 3; ++r)
                for (int q = 0; q < 3; ++q) N[r][q] = (R[r] * G[0][q] + R[3 + r] * G[1][q]) + R[6 + r] * G[2][q];
            for (int r = 0; r < 3; ++r)
                for (int q = r; q < 3; ++q) Gw[r][q] = (N[r][0] * R[q] + N[r][1] * R[3 + q]) + N[r][2] * R[6 + q];
            float* o = g_cov6 + 6 * i;
            o[0] = Gw[0][0]; o[1] = 2.0f * Gw[0][1]; o[2] = 2.0f * Gw[0][2]; o[3] = Gw[1][1]; o[4] = 2.0f * Gw[1][2]; o[5] = Gw[2][2];
        }
        if (g_raw_opacity) {
            const float op = splat[SPLAT_WORDS * i + 5];
            g_raw_opacity[i] = g[5] * (op * (1.0f - op));
        }
        // the colour: a channel clamped at 0 passes nothing
        float gv[3], gd[3];
        for (int ch = 0; ch < 3; ++ch) gv[ch] = splat[SPLAT_WORDS * i + 6 + ch] > 0.0f ? g[6 + ch] : 0.0f;
        float dx = x - cam.cam[0], dy = y - cam.cam[1], dz = z - cam.cam[2];
        const float il = 1.0f / sqrtf((dx * dx + dy * dy) + dz * dz);
        dx *= il; dy *= il; dz *= il;
        sh_colour_bwd(cam.degree, cam.K, sh_rest ? sh_rest + 3 * (int64_t)cam.K * i : nullptr, dx, dy, dz, gv, g_dc ? g_dc + 3 * i : nullptr, o_rest, gd);
        if (g_xyz) {
            // (a, b, c) -> J
            const float u = j11 * Sc[0][1] + j12 * Sc[0][2];
            const float gj00 = 2.0f * (ga * v00) + gb * u, gj02 = 2.0f * (ga * v02) + gb * v12;
            const float gj11 = gb * v01 + 2.0f * (gc * v11), gj12 = gb * v02 + 2.0f * (gc * v12);
            // J and mean2d -> p_c
            const float rz3 = rz2 * rz;
            const float gtx = -(cam.fx * rz2) * gj02, gty = -(cam.fy * rz2) * gj12;
            const float gpx = g[0] * (cam.fx * rz) + (clx ? 0.0f : gtx);
            const float gpy = g[1] * (cam.fy * rz) + (cly ? 0.0f : gty);
            float gpz = -(cam.fx * rz2) * gj00 - (cam.fy * rz2) * gj11;
            gpz = gpz + ((2.0f * (cam.fx * tx)) * rz3) * gj02;
            gpz = gpz + ((2.0f * (cam.fy * ty)) * rz3) * gj12;
            gpz = gpz - (g[0] * (cam.fx * px)) * rz2;
            gpz = gpz - (g[1] * (cam.fy * py)) * rz2;
            gpz = gpz + (clx ? limx * gtx : 0.0f);
            gpz = gpz + (cly ? limy * gty : 0.0f);
            // the unit direction d = v / |v| -> v: (gd - d (d . gd)) / |v|
            const float dg = (dx * gd[0] + dy * gd[1]) + dz * gd[2];
            const float wx = il * (gd[0] - dx * dg), wy = il * (gd[1] - dy * dg), wz = il * (gd[2] - dz * dg);
            g_xyz[3 * i] = ((R[0] * gpx + R[3] * gpy) + R[6] * gpz) + wx;
            g_xyz[3 * i + 1] = ((R[1] * gpx + R[4] * gpy) + R[7] * gpz) + wy;
            g_xyz[3 * i + 2] = ((R[2] * gpx + R[5] * gpy) + R[8] * gpz) + wz;
        }
    }
}

}  // namespace

struct gsr_raster_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    DevBuf splat, depth, rect, counts, offsets, keys, keys2, vals, vals2, ranges, tmp, counters;
    DevBuf rec;                                   // the backward pass's records: nine floats per intersection
    Event ev[4];
    Event evb[5];                                 // gsr_raster_backward's own: a backward pass leaves the last render's timing alone
    bool timed = false, timed_bwd = false;
    ~gsr_raster_ctx() {     // waits for the stream, then the members free themselves (on the context's device)
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(stream);
    }
};

extern "C" int32_t gsr_raster_create(gsr_raster_ctx** out, int32_t device, void* stream) {
    if (!out) return fail(GSR_E_INVALID, "gsr_raster_create: out is NULL");
    *out = nullptr;
    GSR_TRY(open_device(device, "gsr_raster_create"));
    gsr_raster_ctx* c = new gsr_raster_ctx();
    c->device = device;
    c->stream = (hipStream_t)stream;
    for (Event& e : c->ev)
        if (e.create() != hipSuccess) { delete c; return fail(GSR_E_HIP, "gsr_raster_create: hipEventCreate failed"); }
    for (Event& e : c->evb)
        if (e.create() != hipSuccess) { delete c; return fail(GSR_E_HIP, "gsr_raster_create: hipEventCreate failed"); }
    *out = c;
    return GSR_OK;
}

extern "C" int32_t gsr_raster_destroy(gsr_raster_ctx* c) {
    delete c;       // (NULL: nothing)
    return GSR_OK;
}

// What gsr_raster_backward adds to the arguments of a render: the two incoming gradients and the five outputs (device pointers or NULL).
struct RasterBackward {
    const float *grad_image, *grad_alpha;
    float *g_xyz, *g_cov6, *g_raw_opacity, *g_dc, *g_sh_rest;
};

// The render entries and the backward pass: validation (messages under the caller's name `who`), camera set-up, preprocess, sort, tile
// ranges, then the blend the outputs ask for -- k_raster_blend when `rgb_only` (gsr_raster_render), k_raster_blend_aux otherwise -- or,
// with `bw`, k_raster_blend_bwd and k_raster_splat_bwd (timed by the context's second set of events).
static int32_t raster_run(const char* who, bool rgb_only, gsr_raster_ctx* c, int64_t n, int32_t K, int32_t sh_degree, const float* xyz, const float* cov6,
                          const float* raw_opacity, const float* dc, const float* sh_rest, const float* viewmat, float fx, float fy, float cx, float cy,
                          int32_t width, int32_t height, const float* background, float radius_clip, float* image_out, float* depth_out, float* alpha_out,
                          uint32_t* contribution, int64_t* stats_out, void* stream, const RasterBackward* bw = nullptr) {
    if (!c) return fail(GSR_E_INVALID, "%s: NULL context", who);
    if (n < 0 || n >= ((int64_t)1 << 31) - 1) return fail(GSR_E_INVALID, "%s: n = %lld out of range", who, (long long)n);
    if (sh_degree < 0 || sh_degree > 3 || K < (sh_degree + 1) * (sh_degree + 1) - 1)
        return fail(GSR_E_INVALID, "%s: sh_degree %d needs %d rest coefficients, K = %d", who, sh_degree, (sh_degree + 1) * (sh_degree + 1) - 1, K);
    if (width <= 0 || height <= 0 || width > 16 * 65535 || height > 16 * 65535) return fail(GSR_E_INVALID, "%s: bad image size %d x %d", who, width, height);
    if (!bw && !rgb_only && !image_out && !depth_out && !alpha_out && !contribution) return fail(GSR_E_INVALID, "%s: no output requested", who);
    if (bw && !bw->grad_image && !bw->grad_alpha) return fail(GSR_E_INVALID, "%s: grad_image and grad_alpha are both NULL", who);
    if (bw && !bw->g_xyz && !bw->g_cov6 && !bw->g_raw_opacity && !bw->g_dc && !bw->g_sh_rest) return fail(GSR_E_INVALID, "%s: no output requested", who);
    if (!viewmat || ((rgb_only || image_out || (bw && bw->grad_image)) && !background) || (rgb_only && !image_out) || !(fx > 0.0f) || !(fy > 0.0f))
        return fail(GSR_E_INVALID, "%s: NULL argument or focal length <= 0", who);
    if (n > 0 && (!xyz || !cov6 || !raw_opacity || !dc || (sh_degree > 0 && !sh_rest))) return fail(GSR_E_INVALID, "%s: NULL array", who);
    GSR_HIP(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    Event* ev = bw ? c->evb : c->ev;
    (bw ? c->timed_bwd : c->timed) = false;

    RasterCam cam;
    memset(&cam, 0, sizeof(cam));
    for (int r = 0; r < 3; ++r) {
        for (int q = 0; q < 3; ++q) cam.R[3 * r + q] = viewmat[4 * r + q];
        cam.t[r] = viewmat[4 * r + 3];
    }
    for (int q = 0; q < 3; ++q)          // camera position = -R^T t, float64 from the float32 matrix, narrowed once
        cam.cam[q] = (float)-((double)cam.R[q] * cam.t[0] + (double)cam.R[3 + q] * cam.t[1] + (double)cam.R[6 + q] * cam.t[2]);
    cam.fx = fx; cam.fy = fy; cam.cx = cx; cam.cy = cy;
    const float tan_x = 0.5f * (float)width / fx, tan_y = 0.5f * (float)height / fy;
    cam.lim_xp = ((float)width - cx) / fx + 0.3f * tan_x;
    cam.lim_xn = cx / fx + 0.3f * tan_x;
    cam.lim_yp = ((float)height - cy) / fy + 0.3f * tan_y;
    cam.lim_yn = cy / fy + 0.3f * tan_y;
    cam.near_z = 0.01f; cam.far_z = 1e10f; cam.eps2d = 0.3f; cam.radius_clip = radius_clip;
    cam.W = width; cam.H = height;
    cam.tiles_x = (width + TILE - 1) / TILE; cam.tiles_y = (height + TILE - 1) / TILE;
    cam.degree = sh_degree; cam.K = K;
    const int64_t n_tiles = (int64_t)cam.tiles_x * cam.tiles_y;
    if (n_tiles >= ((int64_t)1 << 31)) return fail(GSR_E_INVALID, "%s: %d x %d has %lld tiles, the tile index is 31 bits", who, width, height, (long long)n_tiles);
    const size_t un = (size_t)n;

    GSR_TRY(c->counters.reserve(4 * sizeof(unsigned long long)));
    GSR_TRY(c->splat.reserve(un * SPLAT_WORDS * sizeof(float)));
    GSR_TRY(c->depth.reserve(un * sizeof(float)));
    GSR_TRY(c->rect.reserve(un * sizeof(ushort4)));
    GSR_TRY(c->counts.reserve((un + 1) * sizeof(int64_t)));
    GSR_TRY(c->offsets.reserve((un + 1) * sizeof(int64_t)));
    GSR_TRY(c->ranges.reserve((size_t)n_tiles * 2 * sizeof(int64_t)));
    size_t scan_bytes = 0;
    GSR_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, c->counts.as<int64_t>(), c->offsets.as<int64_t>(), (int64_t)0, un + 1, rocprim::plus<int64_t>(), st));
    GSR_TRY(c->tmp.reserve(scan_bytes));

    unsigned long long* counters = c->counters.as<unsigned long long>();
    GSR_HIP(hipEventRecord(ev[0], st));
    GSR_HIP(hipMemsetAsync(counters, 0, 4 * sizeof(unsigned long long), st));
    GSR_HIP(hipMemsetAsync(c->counts.as<int64_t>() + n, 0, sizeof(int64_t), st));
    GSR_HIP(hipMemsetAsync(c->ranges.p, 0, (size_t)n_tiles * 2 * sizeof(int64_t), st));
    if (n > 0)
        hipLaunchKernelGGL(k_raster_preprocess, dim3(stride_grid(n)), dim3(256), 0, st, n, cam, xyz, cov6, raw_opacity, dc, sh_rest, c->splat.as<float>(),
                           c->depth.as<float>(), c->rect.as<ushort4>(), c->counts.as<int64_t>(), counters);
    GSR_HIP(rocprim::exclusive_scan(c->tmp.p, scan_bytes, c->counts.as<int64_t>(), c->offsets.as<int64_t>(), (int64_t)0, un + 1, rocprim::plus<int64_t>(), st));
    GSR_HIP(hipEventRecord(ev[1], st));
    // the one host read-back: the total sizes the sort buffers
    int64_t total = 0;
    GSR_HIP(hipMemcpyAsync(&total, c->offsets.as<int64_t>() + n, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    GSR_HIP(hipStreamSynchronize(st));
    if (total < 0) return fail(GSR_E_HIP, "%s: negative intersection count", who);
    GSR_HIP(hipMemcpyAsync(counters + 1, &c->offsets.as<int64_t>()[n], sizeof(int64_t), hipMemcpyDeviceToDevice, st));

    if (total > 0) {
        int tile_bits = 0;
        while (((int64_t)1 << tile_bits) < n_tiles) ++tile_bits;
        const unsigned end_bit = 32u + (unsigned)(tile_bits > 0 ? tile_bits : 1);
        const size_t ut = (size_t)total;
        size_t sort_bytes = 0;
        GSR_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, c->keys.as<uint64_t>(), c->keys2.as<uint64_t>(), c->vals.as<uint32_t>(), c->vals2.as<uint32_t>(), ut,
                                          0u, end_bit, st));
        // what the sort still has to allocate, against what the device has free: an error with the count, not an abort
        auto grow = [](const DevBuf& b, size_t bytes) { return bytes > b.cap ? bytes + bytes / 8 + 256 : (size_t)0; };
        const size_t rec_bytes = bw ? ut * SPLAT_WORDS * sizeof(float) : 0;
        const size_t need = grow(c->keys, ut * 8) + grow(c->keys2, ut * 8) + grow(c->vals, ut * 4) + grow(c->vals2, ut * 4) + grow(c->tmp, sort_bytes) +
                            grow(c->rec, rec_bytes);
        const size_t given_back = (ut * 8 > c->keys.cap ? c->keys.cap : 0) + (ut * 8 > c->keys2.cap ? c->keys2.cap : 0) + (ut * 4 > c->vals.cap ? c->vals.cap : 0) +
                                  (ut * 4 > c->vals2.cap ? c->vals2.cap : 0) + (sort_bytes > c->tmp.cap ? c->tmp.cap : 0) +
                                  (rec_bytes > c->rec.cap ? c->rec.cap : 0);
        size_t free_b = 0, total_b = 0;
        GSR_HIP(hipMemGetInfo(&free_b, &total_b));
        if (need > free_b + given_back)
            return fail(GSR_E_HIP, "%s: %lld splat-tile intersections need %zu more bytes of %s, the device has %zu free", who, (long long)total, need,
                        bw ? "sort and gradient-record buffers" : "sort buffers", free_b + given_back);
        GSR_TRY(c->keys.reserve(ut * 8));
        GSR_TRY(c->keys2.reserve(ut * 8));
        GSR_TRY(c->vals.reserve(ut * 4));
        GSR_TRY(c->vals2.reserve(ut * 4));
        GSR_TRY(c->tmp.reserve(sort_bytes));
        GSR_TRY(c->rec.reserve(rec_bytes));
        hipLaunchKernelGGL(k_raster_emit, dim3(stride_grid(n)), dim3(256), 0, st, n, cam.tiles_x, c->depth.as<float>(), c->rect.as<ushort4>(), c->counts.as<int64_t>(),
                           c->offsets.as<int64_t>(), total, c->keys.as<uint64_t>(), c->vals.as<uint32_t>());
        GSR_HIP(rocprim::radix_sort_pairs(c->tmp.p, sort_bytes, c->keys.as<uint64_t>(), c->keys2.as<uint64_t>(), c->vals.as<uint32_t>(), c->vals2.as<uint32_t>(), ut,
                                          0u, end_bit, st));
        hipLaunchKernelGGL(k_raster_ranges, dim3(stride_grid(total)), dim3(256), 0, st, total, (int32_t)n_tiles, c->keys2.as<uint64_t>(), c->ranges.as<int64_t>(), counters);
    }
    GSR_HIP(hipEventRecord(ev[2], st));
    const dim3 tiles(cam.tiles_x, cam.tiles_y);
    const float bg[3] = {background ? background[0] : 0.0f, background ? background[1] : 0.0f, background ? background[2] : 0.0f};
    if (bw) {
        if (total > 0)
            hipLaunchKernelGGL(k_raster_blend_bwd, tiles, dim3(BLEND_THREADS), 0, st, width, height, cam.tiles_x, bg[0], bg[1], bg[2], n, c->ranges.as<int64_t>(),
                               c->vals2.as<uint32_t>(), c->splat.as<float>(), c->rect.as<ushort4>(), c->offsets.as<int64_t>(), total, bw->grad_image,
                               bw->grad_alpha, c->rec.as<float>());
        GSR_HIP(hipEventRecord(ev[3], st));
        if (n > 0)
            hipLaunchKernelGGL(k_raster_splat_bwd, dim3(stride_grid(n)), dim3(256), 0, st, n, cam, xyz, cov6, sh_rest, c->splat.as<float>(), c->counts.as<int64_t>(),
                               c->offsets.as<int64_t>(), c->rec.as<float>(), bw->g_xyz, bw->g_cov6, bw->g_raw_opacity, bw->g_dc, bw->g_sh_rest);
        GSR_HIP(hipEventRecord(ev[4], st));
        if (stats_out) GSR_HIP(hipMemcpyAsync(stats_out, counters, 3 * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        GSR_HIP(hipGetLastError());
        c->timed_bwd = true;
        return GSR_OK;
    }
    if (rgb_only)
        hipLaunchKernelGGL(k_raster_blend, tiles, dim3(BLEND_THREADS), 0, st, width, height, cam.tiles_x, bg[0], bg[1], bg[2], n, c->ranges.as<int64_t>(),
                           c->vals2.as<uint32_t>(), c->splat.as<float>(), image_out);
    else if (contribution)
        hipLaunchKernelGGL(k_raster_blend_aux<true>, tiles, dim3(BLEND_THREADS), 0, st, width, height, cam.tiles_x, bg[0], bg[1], bg[2], n,
                           c->ranges.as<int64_t>(), c->vals2.as<uint32_t>(), c->splat.as<float>(), c->depth.as<float>(), image_out, depth_out, alpha_out,
                           contribution);
    else
        hipLaunchKernelGGL(k_raster_blend_aux<false>, tiles, dim3(BLEND_THREADS), 0, st, width, height, cam.tiles_x, bg[0], bg[1], bg[2], n,
                           c->ranges.as<int64_t>(), c->vals2.as<uint32_t>(), c->splat.as<float>(), c->depth.as<float>(), image_out, depth_out, alpha_out,
                           (uint32_t*)nullptr);
    GSR_HIP(hipEventRecord(ev[3], st));
    if (stats_out) GSR_HIP(hipMemcpyAsync(stats_out, counters, 3 * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    GSR_HIP(hipGetLastError());
    c->timed = true;
    return GSR_OK;
}

extern "C" int32_t gsr_raster_render(gsr_raster_ctx* c, int64_t n, int32_t K, int32_t sh_degree, const float* xyz, const float* cov6, const float* raw_opacity,
                                     const float* dc, const float* sh_rest, const float* viewmat, float fx, float fy, float cx, float cy, int32_t width,
                                     int32_t height, const float* background, float radius_clip, float* image_out, int64_t* stats_out, void* stream) {
    return raster_run("gsr_raster_render", true, c, n, K, sh_degree, xyz, cov6, raw_opacity, dc, sh_rest, viewmat, fx, fy, cx, cy, width, height, background,
                      radius_clip, image_out, nullptr, nullptr, nullptr, stats_out, stream);
}

extern "C" int32_t gsr_raster_render_aux(gsr_raster_ctx* c, int64_t n, int32_t K, int32_t sh_degree, const float* xyz, const float* cov6, const float* raw_opacity,
                                         const float* dc, const float* sh_rest, const float* viewmat, float fx, float fy, float cx, float cy, int32_t width,
                                         int32_t height, const float* background, float radius_clip, float* image_out, float* depth_out, float* alpha_out,
                                         uint32_t* contribution_inout, int64_t* stats_out, void* stream) {
    return raster_run("gsr_raster_render_aux", false, c, n, K, sh_degree, xyz, cov6, raw_opacity, dc, sh_rest, viewmat, fx, fy, cx, cy, width, height, background,
                      radius_clip, image_out, depth_out, alpha_out, contribution_inout, stats_out, stream);
}

extern "C" int32_t gsr_raster_get_timing(gsr_raster_ctx* c, float* ms) {
    if (!c || !ms) return fail(GSR_E_INVALID, "gsr_raster_get_timing: NULL argument");
    if (!c->timed) return fail(GSR_E_INVALID, "gsr_raster_get_timing: no completed render on this context");
    GSR_HIP(hipSetDevice(c->device));
    GSR_HIP(hipEventSynchronize(c->ev[3]));
    for (int i = 0; i < 3; ++i) GSR_HIP(hipEventElapsedTime(&ms[i], c->ev[i], c->ev[i + 1]));
    return GSR_OK;
}

extern "C" int32_t gsr_raster_backward(gsr_raster_ctx* c, int64_t n, int32_t K, int32_t sh_degree, const float* xyz, const float* cov6, const float* raw_opacity,
                                       const float* dc, const float* sh_rest, const float* viewmat, float fx, float fy, float cx, float cy, int32_t width,
                                       int32_t height, const float* background, float radius_clip, const float* grad_image, const float* grad_alpha,
                                       float* grad_xyz, float* grad_cov6, float* grad_raw_opacity, float* grad_dc, float* grad_sh_rest, int64_t* stats_out,
                                       void* stream) {
    const RasterBackward bw = {grad_image, grad_alpha, grad_xyz, grad_cov6, grad_raw_opacity, grad_dc, grad_sh_rest};
    return raster_run("gsr_raster_backward", false, c, n, K, sh_degree, xyz, cov6, raw_opacity, dc, sh_rest, viewmat, fx, fy, cx, cy, width, height, background,
                      radius_clip, nullptr, nullptr, nullptr, nullptr, stats_out, stream, &bw);
}

extern "C" int32_t gsr_raster_get_backward_timing(gsr_raster_ctx* c, float* ms) {
    if (!c || !ms) return fail(GSR_E_INVALID, "gsr_raster_get_backward_timing: NULL argument");
    if (!c->timed_bwd) return fail(GSR_E_INVALID, "gsr_raster_get_backward_timing: no completed backward pass on this context");
    GSR_HIP(hipSetDevice(c->device));
    GSR_HIP(hipEventSynchronize(c->evb[4]));
    for (int i = 0; i < 4; ++i) GSR_HIP(hipEventElapsedTime(&ms[i], c->evb[i], c->evb[i + 1]));
    return GSR_OK;
}

// ---- image metrics ---------------------------------------------------------------------------------------------------------------
namespace {

constexpr int MT = 16, WIN = 11, HALO = 5, MTH = MT + 2 * HALO;       // 16 x 16 pixels per group, 26 x 26 with the halo

struct SsimWindow { double w[WIN]; };

// One group per 16 x 16 tile of one channel.  The halo of both images goes to LDS (zeros outside: the padding of the convolution),
// a horizontal pass leaves the five moment rows (a, b, a a, b b, a b) in LDS, the vertical pass gives every pixel its SSIM term.
// float64 throughout; the group's sums are folded in a fixed tree and written to partial[2 g], partial[2 g + 1].
__global__ __launch_bounds__(MT * MT) void k_metrics_tiles(int32_t H, int32_t W, SsimWindow win, const float* __restrict__ A, const float* __restrict__ B,
                                                           double* __restrict__ partial) {
    __shared__ float s_a[MTH][MTH + 1], s_b[MTH][MTH + 1];
    __shared__ double s_m[5][MTH][MT];
    __shared__ double s_red[2][MT * MT];
    const int t = threadIdx.x, lx = t & (MT - 1), ly = t >> 4;
    const int x0 = blockIdx.x * MT, y0 = blockIdx.y * MT;
    const int64_t plane = (int64_t)blockIdx.z * H * W;
    for (int k = t; k < MTH * MTH; k += MT * MT) {
        const int r = k / MTH, q = k - r * MTH;
        const int y = y0 + r - HALO, x = x0 + q - HALO;
        const bool in = y >= 0 && y < H && x >= 0 && x < W;
        s_a[r][q] = in ? A[plane + (int64_t)y * W + x] : 0.0f;
        s_b[r][q] = in ? B[plane + (int64_t)y * W + x] : 0.0f;
    }
    __syncthreads();
    for (int k = t; k < MTH * MT; k += MT * MT) {
        const int r = k / MT, q = k - r * MT;
        double m0 = 0, m1 = 0, m2 = 0, m3 = 0, m4 = 0;
        for (int j = 0; j < WIN; ++j) {
            const double a = (double)s_a[r][q + j], b = (double)s_b[r][q + j], w = win.w[j];
            m0 += w * a; m1 += w * b; m2 += w * (a * a); m3 += w * (b * b); m4 += w * (a * b);
        }
        s_m[0][r][q] = m0; s_m[1][r][q] = m1; s_m[2][r][q] = m2; s_m[3][r][q] = m3; s_m[4][r][q] = m4;
    }
    __syncthreads();
    double ssim = 0.0, se = 0.0;
    if (x0 + lx < W && y0 + ly < H) {
        double m[5] = {0, 0, 0, 0, 0};
        for (int j = 0; j < WIN; ++j)
            for (int k = 0; k < 5; ++k) m[k] += win.w[j] * s_m[k][ly + j][lx];
        const double mu1 = m[0], mu2 = m[1], mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
        const double s1 = m[2] - mu1_sq, s2 = m[3] - mu2_sq, s12 = m[4] - mu12;
        const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
        ssim = ((2.0 * mu12 + C1) * (2.0 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2));
        const float d = s_a[ly + HALO][lx + HALO] - s_b[ly + HALO][lx + HALO];      // the difference in float32, as the reference takes it
        se = (double)d * (double)d;
    }
    s_red[0][t] = ssim; s_red[1][t] = se;
    __syncthreads();
    for (int s = MT * MT / 2; s > 0; s >>= 1) {
        if (t < s) { s_red[0][t] += s_red[0][t + s]; s_red[1][t] += s_red[1][t + s]; }
        __syncthreads();
    }
    if (t == 0) {
        const int64_t g = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        partial[2 * g] = s_red[0][0]; partial[2 * g + 1] = s_red[1][0];
    }
}

// second stage: one group, every thread a strided slice in ascending order, then the same fixed tree.  out = (mse, ssim)
__global__ __launch_bounds__(256) void k_metrics_final(int64_t groups, double count, const double* __restrict__ partial, double* __restrict__ out) {
    __shared__ double s_red[2][256];
    const int t = threadIdx.x;
    double a = 0.0, b = 0.0;
    for (int64_t g = t; g < groups; g += 256) { a += partial[2 * g]; b += partial[2 * g + 1]; }
    s_red[0][t] = a; s_red[1][t] = b;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) { s_red[0][t] += s_red[0][t + s]; s_red[1][t] += s_red[1][t + s]; }
        __syncthreads();
    }
    if (t == 0) { out[0] = s_red[1][0] / count; out[1] = s_red[0][0] / count; }
}

}  // namespace

extern "C" int32_t gsr_image_metrics(const float* a, const float* b, int32_t height, int32_t width, int32_t on_device, double* out, int32_t device, void* stream) {
    if (!a || !b || !out || height <= 0 || width <= 0) return fail(GSR_E_INVALID, "gsr_image_metrics: bad argument");
    GSR_TRY(open_device(device, "gsr_image_metrics"));
    SsimWindow win;
    double sum = 0.0;
    for (int j = 0; j < WIN; ++j) { win.w[j] = exp(-(double)((j - WIN / 2) * (j - WIN / 2)) / (2.0 * 1.5 * 1.5)); sum += win.w[j]; }
    for (int j = 0; j < WIN; ++j) win.w[j] /= sum;
    const size_t bytes = (size_t)3 * (size_t)height * (size_t)width * sizeof(float);
    const dim3 grid((width + MT - 1) / MT, (height + MT - 1) / MT, 3);
    if (grid.y > 65535u) return fail(GSR_E_INVALID, "gsr_image_metrics: image too tall");
    const int64_t groups = (int64_t)grid.x * grid.y * grid.z;
    double host[2] = {0.0, 0.0};
    {
        OneShot os((hipStream_t)stream, on_device != 0, "gsr_image_metrics");
        const float *da = nullptr, *db = nullptr;
        double *partial = nullptr, *res = nullptr;
        GSR_TRY(os.in(a, bytes, &da));
        GSR_TRY(os.in(b, bytes, &db));
        GSR_TRY(os.scratch((size_t)groups * 2 * sizeof(double), &partial));
        GSR_TRY(os.scratch(2 * sizeof(double), &res));
        hipLaunchKernelGGL(k_metrics_tiles, grid, dim3(MT * MT), 0, os.st, height, width, win, da, db, partial);
        hipLaunchKernelGGL(k_metrics_final, dim3(1), dim3(256), 0, os.st, groups, 3.0 * (double)height * (double)width, partial, res);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(host, res, sizeof(host), hipMemcpyDeviceToHost, os.st);
        GSR_TRY(os.wait(e));
    }
    out[0] = host[0]; out[1] = host[1];
    return GSR_OK;
}
