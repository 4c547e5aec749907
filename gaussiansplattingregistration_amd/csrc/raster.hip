// raster.hip -- tile rasteriser of a splat model for one pinhole camera, forward and backward (gsr_raster_*), and the image metrics of
// the evaluation stage (gsr_image_metrics).  DESIGN.md sections 14, 22, 26 and 28.
//
// Render: k_raster_preprocess (projection, conic, radius, SH colour, tile count) -> exclusive scan of the 64-bit counts -> ONE
// host read-back of the intersection total -> k_raster_emit (keys (tile id << 32 | depth bits), values = splat index) -> radix
// sort limited to the bits in use (stable: equal depths keep ascending splat index) -> k_raster_ranges -> k_raster_blend<MODE>, one
// 256-thread work-group per 16 x 16 tile.  No float atomics: every pixel sums its splats front to back in the sorted order, so
// an image is the same bits from run to run.  The two counters (visible splats, non-empty tiles) are integer atomics.
//
// The semantics restate the published 3DGS / gsplat forward pass (EWA projection with the clamped perspective Jacobian, 0.3 px
// dilation, 3-sigma integer radius, alpha clamp 0.999, 1/255 skip, transmittance stop at 1e-4); gsplat itself is not available on
// ROCm, so parity with it is unpinned.  tests/raster_model.py is the executable restatement the kernels are held to.
//
// gsr_raster_render_aux is the same pipeline with another mode of the blend: coverage 1 - T, expected depth
// sum(z w) / alpha and, per splat, the largest blending weight w = alpha T it reaches on any pixel (an integer atomicMax on the
// float's bits: still no float atomics).  tests/raster_aux_model.py restates it.
//
// gsr_raster_backward is the backward pass of that render: the same pipeline up to the tile ranges, then
// k_raster_blend_bwd (one record of nine floats per splat-tile intersection, folded over the tile in a fixed tree) and k_raster_splat_bwd
// (every splat adds its records in a fixed order and runs the projection backwards).  No float atomics either; tests/raster_grad_model.py
// restates it.
//
// Every part of the semantics is written once: splat_at_pixel (what a staged splat is to a pixel), walk_batch (the
// front-to-back walk and its stop), tile_pixel / post_alive / stage_batch (a tile's set-up and its LDS batches), cam_point /
// project_splat / view_direction (the camera-space chain, forward values for both directions), sh_basis (the SH polynomials and
// their derivatives) and wave_ladder (the DPP steps of both wave reductions).
#include <math.h>
#include <string.h>

#include <rocprim/rocprim.hpp>

#include "gsr_common.h"
#include "gsr_oneshot.h"
#include "gsr_ssim_window.h"

using namespace gsr;

namespace {

constexpr int TILE = 16;
constexpr int BLEND_THREADS = TILE * TILE;          // four waves
constexpr int SPLAT_WORDS = 9;                      // mean2d xy, conic A B C, opacity, r g b: 36 bytes
constexpr float ALPHA_MAX = 0.999f;                 // the clamp of a splat's alpha on a pixel
constexpr float ALPHA_MIN = 1.0f / 255.0f;          // below it a splat does not count for the pixel
constexpr float T_STOP = 1e-4f;                     // a pixel is finished before the splat that would take its transmittance this low

struct RasterCam {
    float R[9], t[3], cam[3];                       // world -> camera rotation (row-major), translation; camera position in the world
    float fx, fy, cx, cy;
    float lim_xp, lim_xn, lim_yp, lim_yn;           // the frustum in x/z, y/z widened by 0.3 tan(fov/2) on each side
    float near_z, far_z, eps2d, radius_clip;
    int32_t W, H, tiles_x, tiles_y, degree, K;
};

// ---- the camera-space chain: k_raster_preprocess forms these values, k_raster_splat_bwd differentiates them -------------------------
struct CamPoint { float x, y, z; };

__device__ __forceinline__ CamPoint cam_point(const RasterCam& cam, float x, float y, float z) {
    const float* R = cam.R;
    return {((R[0] * x + R[1] * y) + R[2] * z) + cam.t[0], ((R[3] * x + R[4] * y) + R[5] * z) + cam.t[1], ((R[6] * x + R[7] * y) + R[8] * z) + cam.t[2]};
}

// Sigma_c = R S R^T, the perspective Jacobian J at the clamped (tx, ty), V = Sigma_c J^T, the dilated 2-D covariance (a b; b c) and the mean
struct Projected {
    float Sc[3][3];
    float rz, rz2, tx, ty;
    float j00, j02, j11, j12;
    float v00, v01, v02, v11, v12;
    float a, b, c, det, mx, my;
};

__device__ __forceinline__ void project_splat(const RasterCam& cam, const float* s, const CamPoint& p, Projected& P) {
    const float* R = cam.R;
    const float S[3][3] = {{s[0], s[1], s[2]}, {s[1], s[3], s[4]}, {s[2], s[4], s[5]}};
    float M[3][3];
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) M[r][q] = (R[3 * r] * S[0][q] + R[3 * r + 1] * S[1][q]) + R[3 * r + 2] * S[2][q];
    for (int r = 0; r < 3; ++r)
        for (int q = r; q < 3; ++q) P.Sc[r][q] = P.Sc[q][r] = (M[r][0] * R[3 * q] + M[r][1] * R[3 * q + 1]) + M[r][2] * R[3 * q + 2];
    P.rz = 1.0f / p.z;
    P.tx = p.z * fminf(cam.lim_xp, fmaxf(-cam.lim_xn, p.x * P.rz));
    P.ty = p.z * fminf(cam.lim_yp, fmaxf(-cam.lim_yn, p.y * P.rz));
    P.rz2 = P.rz * P.rz;
    P.j00 = cam.fx * P.rz; P.j02 = -(cam.fx * P.tx) * P.rz2; P.j11 = cam.fy * P.rz; P.j12 = -(cam.fy * P.ty) * P.rz2;
    P.v00 = P.Sc[0][0] * P.j00 + P.Sc[0][2] * P.j02; P.v01 = P.Sc[1][0] * P.j00 + P.Sc[1][2] * P.j02; P.v02 = P.Sc[2][0] * P.j00 + P.Sc[2][2] * P.j02;
    P.v11 = P.Sc[1][1] * P.j11 + P.Sc[1][2] * P.j12; P.v12 = P.Sc[2][1] * P.j11 + P.Sc[2][2] * P.j12;
    P.a = (P.j00 * P.v00 + P.j02 * P.v02) + cam.eps2d;
    P.b = P.j11 * P.v01 + P.j12 * P.v02;
    P.c = (P.j11 * P.v11 + P.j12 * P.v12) + cam.eps2d;
    P.det = P.a * P.c - P.b * P.b;
    P.mx = (cam.fx * p.x) * P.rz + cam.cx;
    P.my = (cam.fy * p.y) * P.rz + cam.cy;
}

// d = the unit vector from the camera to the splat; returns 1 / |splat - camera|
__device__ __forceinline__ float view_direction(const RasterCam& cam, float x, float y, float z, float* d) {
    const float dx = x - cam.cam[0], dy = y - cam.cam[1], dz = z - cam.cam[2];
    const float il = 1.0f / sqrtf((dx * dx + dy * dy) + dz * dz);
    d[0] = dx * il; d[1] = dy * il; d[2] = dz * il;
    return il;
}

// ---- the SH basis 3DGS evaluates ---------------------------------------------------------------------------------------------------
constexpr float SH_C0 = 0.28209479177387814f;       // the constant basis function: the DC term is SH_C0 * dc

// term(k, b_k, db_k/dx, db_k/dy, db_k/dz) for the coefficients k = 0 .. nb - 1 of the degree, in ascending k, at the unit vector
// (x, y, z); returns nb.  A visitor that ignores the derivatives pays nothing for them.
template <typename F>
__device__ __forceinline__ int sh_basis(int degree, float x, float y, float z, F term) {
    const float C1 = 0.4886025119029199f;
    const float C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f, -1.0925484305920792f, 0.5462742152960396f};
    const float C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f, 0.3731763325901154f, -0.4570457994644658f, 1.445305721320277f,
                         -0.5900435899266435f};
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
    return nb;
}

// SH colour; rest[k*3 + c], k = 0 .. K-1 (coefficient-major).  d is a unit vector.  Every channel adds its terms in ascending k.
__device__ __forceinline__ void sh_colour(int degree, const float* __restrict__ dc, const float* __restrict__ rest, float x, float y, float z, float* rgb) {
    float b[15];
    const int nb = sh_basis(degree, x, y, z, [&](int k, float bk, float, float, float) { b[k] = bk; });
    for (int c = 0; c < 3; ++c) {
        float v = SH_C0 * dc[c];
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
            const CamPoint p = cam_point(cam, x, y, z);
            bool ok = p.z >= cam.near_z && p.z <= cam.far_z;
            Projected P;
            float rad = 0.f;
            if (ok) {
                project_splat(cam, cov6 + 6 * i, p, P);
                ok = P.det > 0.0f;
            }
            if (ok) {
                const float bm = 0.5f * (P.a + P.c);
                rad = ceilf(3.0f * sqrtf(bm + sqrtf(fmaxf(0.01f, bm * bm - P.det))));
                ok = rad > cam.radius_clip && !(P.mx + rad <= 0.0f || P.mx - rad >= (float)cam.W || P.my + rad <= 0.0f || P.my - rad >= (float)cam.H);
            }
            if (ok) {
                const float inv = 1.0f / (float)TILE;
                // clamped as floats: a far-off mean or a huge radius must not reach the conversion to int
                const float fx_t = (float)cam.tiles_x, fy_t = (float)cam.tiles_y;
                const int x0 = (int)fminf(fmaxf(floorf((P.mx - rad) * inv), 0.0f), fx_t), x1 = (int)fminf(fmaxf(ceilf((P.mx + rad) * inv), 0.0f), fx_t);
                const int y0 = (int)fminf(fmaxf(floorf((P.my - rad) * inv), 0.0f), fy_t), y1 = (int)fminf(fmaxf(ceilf((P.my + rad) * inv), 0.0f), fy_t);
                touched = (int64_t)(x1 - x0) * (int64_t)(y1 - y0);
                ok = touched > 0;
                if (ok) {
                    float d[3], rgb[3];
                    view_direction(cam, x, y, z, d);
                    sh_colour(cam.degree, dc + 3 * i, sh_rest ? sh_rest + 3 * (int64_t)cam.K * i : nullptr, d[0], d[1], d[2], rgb);
                    float* o = splat + SPLAT_WORDS * i;
                    o[0] = P.mx; o[1] = P.my;
                    o[2] = P.c / P.det; o[3] = -P.b / P.det; o[4] = P.a / P.det;
                    o[5] = 1.0f / (1.0f + expf(-raw_opacity[i]));
                    o[6] = rgb[0]; o[7] = rgb[1]; o[8] = rgb[2];
                    depth[i] = p.z;
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

// ---- what the blend kernels share ----------------------------------------------------------------------------------------------------
// One work-group per tile, one thread per pixel (wave w holds rows 4 w .. 4 w + 3); [first, last) are the tile's sorted positions.
struct TilePixel {
    int t, wave, lane, ix, iy;
    bool inside;
    float px, py;                                   // the pixel centre
    int64_t first, last;
};

__device__ __forceinline__ TilePixel tile_pixel(int32_t W, int32_t H, int32_t tiles_x, const int64_t* __restrict__ ranges) {
    TilePixel p;
    p.t = threadIdx.x; p.wave = p.t >> 6; p.lane = p.t & 63;
    const int tile = blockIdx.y * tiles_x + blockIdx.x;
    p.ix = blockIdx.x * TILE + (p.t & (TILE - 1)); p.iy = blockIdx.y * TILE + (p.t >> 4);
    p.inside = p.ix < W && p.iy < H;
    p.px = (float)p.ix + 0.5f; p.py = (float)p.iy + 0.5f;
    p.first = ranges[2 * (int64_t)tile]; p.last = ranges[2 * (int64_t)tile + 1];
    return p;
}

// Before a batch's first barrier every wave posts whether any of its lanes still has work in s_alive[wave] and gets its own answer
// back: a wave without one skips the batch, and when all four say so (any_alive, after the barrier) the group leaves.
__device__ __forceinline__ bool post_alive(int* s_alive, const TilePixel& p, bool lane_alive) {
    const bool wave_alive = __ballot(lane_alive) != 0ull;
    if (p.lane == 0) s_alive[p.wave] = wave_alive ? 1 : 0;
    return wave_alive;
}

__device__ __forceinline__ bool any_alive(const int* s_alive) { return (s_alive[0] | s_alive[1] | s_alive[2] | s_alive[3]) != 0; }

// Thread t stages the first WORDS words of the splat at sorted position pos < end in s_splat[9 t ..] (stride 9 words: conflict-free
// writes, broadcast reads) and returns its index, or -1 where there is none: behind the end, or never, an index the emit kernel did
// not write (zeros are staged then).
template <int WORDS>
__device__ __forceinline__ int64_t stage_batch(float* s_splat, int t, int64_t pos, int64_t end, const uint32_t* __restrict__ vals, int64_t n,
                                               const float* __restrict__ splat) {
    if (pos >= end) return -1;
    const uint32_t id = vals[pos];
    if ((int64_t)id < n) {
        const float* src = splat + (int64_t)SPLAT_WORDS * id;
#pragma unroll
        for (int k = 0; k < WORDS; ++k) s_splat[SPLAT_WORDS * t + k] = src[k];
        return (int64_t)id;
    }
#pragma unroll
    for (int k = 0; k < WORDS; ++k) s_splat[SPLAT_WORDS * t + k] = 0.0f;
    return -1;
}

__device__ __forceinline__ int batch_size(int64_t left) { return (int)(left < (int64_t)BLEND_THREADS ? left : (int64_t)BLEND_THREADS); }

// What the staged splat s is to the pixel centred at (px, py): its offset, e = exp(-sigma), araw = opacity e, alpha = araw clamped, and
// whether it counts at all (sigma >= 0 and alpha >= 1/255; where it does not, e, araw and alpha are not formed).
struct SplatAtPixel {
    float dx, dy, e, araw, alpha;
    bool counts;
};

__device__ __forceinline__ SplatAtPixel splat_at_pixel(const float* s, float px, float py) {
    SplatAtPixel q;
    q.dx = s[0] - px; q.dy = s[1] - py;
    q.e = q.araw = q.alpha = 0.0f;
    q.counts = false;
    const float sigma = 0.5f * (s[2] * q.dx * q.dx + s[4] * q.dy * q.dy) + s[3] * q.dx * q.dy;
    if (!(sigma < 0.0f)) {
        const float opacity = s[5];                 // read ahead of the exponential: its LDS latency hides behind it
        q.e = expf(-sigma);
        q.araw = opacity * q.e;
        q.alpha = fminf(ALPHA_MAX, q.araw);
        q.counts = !(q.alpha < ALPHA_MIN);
    }
    return q;
}

// The front-to-back walk of one staged batch of m splats by one pixel: counted(j, alpha, T) for every splat that counts, T being
// the transmittance in front of it; the pixel is done, and leaves, at the first splat that would take T to T_STOP or below.
template <typename F>
__device__ __forceinline__ void walk_batch(const float* s_splat, int m, float px, float py, float& T, bool& done, F counted) {
    for (int j = 0; j < m && !done; ++j) {
        const SplatAtPixel q = splat_at_pixel(s_splat + SPLAT_WORDS * j, px, py);
        if (!q.counts) continue;
        const float Tn = T * (1.0f - q.alpha);
        if (Tn <= T_STOP) { done = true; break; }
        counted(j, q.alpha, T);
        T = Tn;
    }
}

// The six DPP steps of a wave reduction: four row_shr steps leave each row of 16 lanes its inclusive results, row_bcast15 and
// row_bcast31 carry the row ends across, so lane 63 holds op over the wave as the tree of adjacent pairs
// ((x15 op x14) op (x13 op x12)) op ... per row, rows 0 and 1, rows 2 and 3, then the halves.  A lane without a source takes `old` = 0
// bits, which must be op's identity.  All 64 lanes must be active.
template <int CTRL, int ROW_MASK, typename V, typename Op>
__device__ __forceinline__ V dpp_step(V v, Op op) {
    static_assert(sizeof(V) == sizeof(int), "one DPP word");
    return op(v, __builtin_bit_cast(V, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, false)));
}

template <typename V, typename Op>
__device__ __forceinline__ V wave_ladder(V v, Op op) {
    v = dpp_step<0x111, 0xf>(v, op);      // row_shr:1
    v = dpp_step<0x112, 0xf>(v, op);      // row_shr:2
    v = dpp_step<0x114, 0xf>(v, op);      // row_shr:4
    v = dpp_step<0x118, 0xf>(v, op);      // row_shr:8
    v = dpp_step<0x142, 0xa>(v, op);      // row_bcast15 into rows 1, 3
    v = dpp_step<0x143, 0xc>(v, op);      // row_bcast31 into rows 2, 3
    return v;
}

// The largest value of a wave, in every lane (0 is the identity of a maximum of unsigned values).
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_readlane((int)wave_ladder(v, [](uint32_t a, uint32_t b) { return a > b ? a : b; }), 63);
}

// The sum of a wave, valid in lane 63 (a lane without a source adds +0.0).  One row is one pixel row of the tile, a wave four of them.
__device__ __forceinline__ float wave_sum_f32(float v) {
    return wave_ladder(v, [](float a, float b) { return a + b; });
}

// The forward blend.  Batches of 256 sorted splats are staged in LDS and walked by every pixel that is not done.  BLEND_RGB writes the
// image.  BLEND_AUX walks the same loop in the same float32 order (a requested image is the bits BLEND_RGB writes) and adds
// D = sum z w per pixel (s_z: the tenth staged word, kept out of the stride-9 record); image, depth, alpha: each NULL or written
// (wave-uniform tests).  BLEND_AUX_CONTRIB also raises the largest w = alpha T of every staged splat: s_contrib[j] belongs to the thread
// that staged splat j, which zeroes it, lets the waves raise it between the barriers and sends it to contribution[id] with one integer
// atomicMax after the closing barrier (non-negative floats order as their bit patterns: no float atomics, no dependence on the order).
// There the j loop is wave-uniform -- it runs while any lane is live, finished lanes offer 0 -- so that the wave's maximum is taken by
// DPP steps and one lane raises the slot.  A mode carries nothing of what it does not have: s_z and s_contrib are not allocated.
enum BlendMode { BLEND_RGB, BLEND_AUX, BLEND_AUX_CONTRIB };

template <BlendMode MODE>
__global__ __launch_bounds__(BLEND_THREADS) void k_raster_blend(int32_t W, int32_t H, int32_t tiles_x, float bg0, float bg1, float bg2, int64_t n,
                                                                const int64_t* __restrict__ ranges, const uint32_t* __restrict__ vals,
                                                                const float* __restrict__ splat, const float* __restrict__ zs, float* __restrict__ image,
                                                                float* __restrict__ depth, float* __restrict__ alpha_out, uint32_t* __restrict__ contribution) {
    constexpr bool AUX = MODE != BLEND_RGB, CONTRIB = MODE == BLEND_AUX_CONTRIB;
    __shared__ float s_splat[BLEND_THREADS * SPLAT_WORDS];
    __shared__ float s_z[BLEND_THREADS];
    __shared__ uint32_t s_contrib[BLEND_THREADS];
    __shared__ int s_alive[BLEND_THREADS / 64];
    const TilePixel p = tile_pixel(W, H, tiles_x, ranges);
    float T = 1.0f, r = 0.0f, g = 0.0f, b = 0.0f, D = 0.0f;
    bool done = !p.inside;
    // a counted splat adds its colour (and depth) with the weight w = alpha T, which is returned
    auto add = [&](int j, float alpha, float T_front) {
        const float* s = s_splat + SPLAT_WORDS * j;
        const float vis = alpha * T_front;
        r = r + s[6] * vis; g = g + s[7] * vis; b = b + s[8] * vis;
        if constexpr (AUX) D = D + s_z[j] * vis;
        return vis;
    };
    for (int64_t base = p.first; base < p.last; base += BLEND_THREADS) {
        const bool wave_alive = post_alive(s_alive, p, !done);
        const int64_t my_id = stage_batch<SPLAT_WORDS>(s_splat, p.t, base + p.t, p.last, vals, n, splat);      // reported to, if not -1
        if constexpr (AUX) s_z[p.t] = my_id >= 0 ? zs[my_id] : 0.0f;
        if constexpr (CONTRIB) s_contrib[p.t] = 0u;
        __syncthreads();
        if (!any_alive(s_alive)) break;                                // (every slot is still zero: nothing to send)
        if (wave_alive) {
            const int m = batch_size(p.last - base);
            if constexpr (CONTRIB) {
                for (int j = 0; j < m; ++j) {
                    if (__ballot(!done) == 0ull) break;
                    float w = 0.0f;
                    if (!done) {
                        const SplatAtPixel q = splat_at_pixel(s_splat + SPLAT_WORDS * j, p.px, p.py);
                        if (q.counts) {
                            const float Tn = T * (1.0f - q.alpha);
                            if (Tn <= T_STOP) done = true;
                            else { w = add(j, q.alpha, T); T = Tn; }
                        }
                    }
                    const uint32_t top = wave_max_u32(__float_as_uint(w));       // w >= 0: its bits order as it does
                    if (top != 0u && p.lane == 0) atomicMax(&s_contrib[j], top);
                }
            } else {
                walk_batch(s_splat, m, p.px, p.py, T, done, add);
            }
        }
        __syncthreads();
        if constexpr (CONTRIB) {
            if (my_id >= 0) {
                const uint32_t top = s_contrib[p.t];
                if (top != 0u) atomicMax(contribution + my_id, top);
            }
        }
    }
    if (p.inside) {
        const int64_t at = (int64_t)p.iy * W + p.ix;
        bool want_image = true;
        if constexpr (AUX) want_image = image != nullptr;
        if (want_image) {
            float* o = image + 3 * at;
            o[0] = r + T * bg0; o[1] = g + T * bg1; o[2] = b + T * bg2;
        }
        if constexpr (AUX) {
            const float a = 1.0f - T;
            if (alpha_out) alpha_out[at] = a;
            if (depth) depth[at] = D / fmaxf(a, 1e-10f);
        }
    }
}

// ---- backward pass (gsr_raster_backward) -------------------------------------------------------------------
// One work-group per tile, one thread per pixel, as the forward.  First the forward walk (walk_batch over the six words it needs, no
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
    const TilePixel p = tile_pixel(W, H, tiles_x, ranges);
    const int t = p.t, wave = p.wave, lane = p.lane;
    const float px = p.px, py = p.py;
    const int64_t first = p.first, last = p.last;
    if (first >= last) return;
    if (t == 0) s_count = 0;
    float T = 1.0f;
    int last_cnt = -1;                                             // offset from `first` of the last splat this pixel counted
    bool done = !p.inside;
    for (int64_t base = first; base < last; base += BLEND_THREADS) {
        const bool wave_alive = post_alive(s_alive, p, !done);
        stage_batch<6>(s_splat, t, base + t, last, vals, n, splat);
        __syncthreads();
        if (!any_alive(s_alive)) break;
        if (wave_alive)
            walk_batch(s_splat, batch_size(last - base), px, py, T, done, [&](int j, float, float) { last_cnt = (int)(base - first) + j; });
        __syncthreads();
    }
    if (last_cnt >= 0) atomicMax(&s_count, last_cnt + 1);         // an integer maximum in LDS
    __syncthreads();
    const int count = s_count;                                     // positions first .. first + count - 1 are walked back
    // where the record of a sorted position goes: the slot k_raster_emit gave this (splat, tile) pair, offsets[id] + the tile's row-major
    // index in the splat's box -- the inverse of the sort, computed instead of stored.  -1: never (an index the emit kernel did not write)
    const int tile_x = blockIdx.x, tile_y = blockIdx.y;
    auto slot_of = [&](int64_t id) -> int64_t {
        if (id < 0 || id >= n) return -1;
        const ushort4 r = rect[id];
        if (tile_x < r.x || tile_x >= r.z || tile_y < r.y || tile_y >= r.w) return -1;
        const int64_t slot = offsets[id] + (int64_t)(tile_y - r.y) * (r.z - r.x) + (tile_x - r.x);
        return slot < total ? slot : -1;
    };
    for (int64_t pos = first + count + t; pos < last; pos += BLEND_THREADS) {
        const int64_t slot = slot_of((int64_t)vals[pos]);
        if (slot >= 0) {
#pragma unroll
            for (int k = 0; k < SPLAT_WORDS; ++k) rec[SPLAT_WORDS * slot + k] = 0.0f;
        }
    }

    float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f, gA = 0.0f;
    if (p.inside) {
        const int64_t at = (int64_t)p.iy * W + p.ix;
        if (grad_image) { g0 = grad_image[3 * at]; g1 = grad_image[3 * at + 1]; g2 = grad_image[3 * at + 2]; }
        if (grad_alpha) gA = grad_alpha[at];
    }
    const float T_end = T;
    const float tga = T_end * gA;
    float acc = T_end * ((bg0 * g0 + bg1 * g1) + bg2 * g2);
    for (int b = (count - 1) / BLEND_THREADS; b >= 0 && count > 0; --b) {
        const int off0 = b * BLEND_THREADS;
        const int m = batch_size(count - off0);
        const bool wave_live = post_alive(s_alive, p, last_cnt >= off0);
        const int64_t my_slot = slot_of(stage_batch<SPLAT_WORDS>(s_splat, t, first + off0 + t, first + count, vals, n, splat));
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
                    const SplatAtPixel q = splat_at_pixel(s, px, py);
                    if (q.counts) {
                        counted = true;
                        const float om = 1.0f - q.alpha;
                        T = T / om;
                        const float w = q.alpha * T;
                        const float cg = (s[6] * g0 + s[7] * g1) + s[8] * g2;
                        v[6] = w * g0; v[7] = w * g1; v[8] = w * g2;
                        const float dalpha = T * cg - (acc - tga) / om;
                        acc = acc + w * cg;
                        if (!(q.araw > ALPHA_MAX)) {                           // not clamped: sigma and the opacity take part
                            v[5] = q.e * dalpha;
                            const float gs = -(q.alpha * dalpha);
                            v[0] = gs * (s[2] * q.dx + s[3] * q.dy);
                            v[1] = gs * (s[4] * q.dy + s[3] * q.dx);
                            v[2] = gs * (0.5f * (q.dx * q.dx));
                            v[3] = gs * (q.dx * q.dy);
                            v[4] = gs * (0.5f * (q.dy * q.dy));
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
// or written: coefficients beyond the degree get 0) and gd = dL/d(unit direction) through the basis.
__device__ __forceinline__ void sh_colour_bwd(int degree, int K, const float* __restrict__ rest, float x, float y, float z, const float* gv,
                                              float* __restrict__ g_dc, float* __restrict__ g_rest, float* gd) {
    if (g_dc) { g_dc[0] = SH_C0 * gv[0]; g_dc[1] = SH_C0 * gv[1]; g_dc[2] = SH_C0 * gv[2]; }
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
    const int nb = sh_basis(degree, x, y, z, [&](int k, float bk, float ddx, float ddy, float ddz) {
        const float* r = rest + 3 * k;
        const float gb = (r[0] * gv[0] + r[1] * gv[1]) + r[2] * gv[2];
        gx = gx + gb * ddx; gy = gy + gb * ddy; gz = gz + gb * ddz;
        if (g_rest) { g_rest[3 * k] = bk * gv[0]; g_rest[3 * k + 1] = bk * gv[1]; g_rest[3 * k + 2] = bk * gv[2]; }
    });
    if (g_rest)
        for (int k = 3 * nb; k < 3 * K; ++k) g_rest[k] = 0.0f;
    gd[0] = gx; gd[1] = gy; gd[2] = gz;
}

// One thread per splat.  A culled splat (counts = 0) writes +0.0 to every output.  A visible one adds the records of the tiles of its rect
// in the order k_raster_emit wrote them (ty outer, tx inner) -- k_raster_blend_bwd left them at the emission's slots, offsets[i] onwards,
// so they are read in a row, without a search -- nine float32 accumulators.  Then the chain of k_raster_preprocess backwards, its forward
// values from the functions the forward calls (opacity and colour are read from the staged splat): conic -> (a, b, c) ->
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
        const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        const float* R = cam.R;
        const CamPoint p = cam_point(cam, x, y, z);
        Projected P;
        project_splat(cam, cov6 + 6 * i, p, P);
        const float rz = P.rz, rz2 = P.rz2, j00 = P.j00, j02 = P.j02, j11 = P.j11, j12 = P.j12, a = P.a, b = P.b, c = P.c;
        // on the clamped branch t = z lim: nothing to x (or y), lim to z
        const float ux = p.x * rz, uy = p.y * rz;
        const bool clx = ux > cam.lim_xp || ux < -cam.lim_xn, cly = uy > cam.lim_yp || uy < -cam.lim_yn;
        const float limx = ux > cam.lim_xp ? cam.lim_xp : -cam.lim_xn, limy = uy > cam.lim_yp ? cam.lim_yp : -cam.lim_yn;
        // conic (c, -b, a) / det -> a, b, c
        const float di = 1.0f / P.det, di2 = di * di;
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
        float gv[3], gd[3], d[3];
        for (int ch = 0; ch < 3; ++ch) gv[ch] = splat[SPLAT_WORDS * i + 6 + ch] > 0.0f ? g[6 + ch] : 0.0f;
        const float il = view_direction(cam, x, y, z, d);
        sh_colour_bwd(cam.degree, cam.K, sh_rest ? sh_rest + 3 * (int64_t)cam.K * i : nullptr, d[0], d[1], d[2], gv, g_dc ? g_dc + 3 * i : nullptr, o_rest, gd);
        if (g_xyz) {
            // (a, b, c) -> J
            const float u = j11 * P.Sc[0][1] + j12 * P.Sc[0][2];
            const float gj00 = 2.0f * (ga * P.v00) + gb * u, gj02 = 2.0f * (ga * P.v02) + gb * P.v12;
            const float gj11 = gb * P.v01 + 2.0f * (gc * P.v11), gj12 = gb * P.v02 + 2.0f * (gc * P.v12);
            // J and mean2d -> p_c
            const float rz3 = rz2 * rz;
            const float gtx = -(cam.fx * rz2) * gj02, gty = -(cam.fy * rz2) * gj12;
            const float gpx = g[0] * (cam.fx * rz) + (clx ? 0.0f : gtx);
            const float gpy = g[1] * (cam.fy * rz) + (cly ? 0.0f : gty);
            float gpz = -(cam.fx * rz2) * gj00 - (cam.fy * rz2) * gj11;
            gpz = gpz + ((2.0f * (cam.fx * P.tx)) * rz3) * gj02;
            gpz = gpz + ((2.0f * (cam.fy * P.ty)) * rz3) * gj12;
            gpz = gpz - (g[0] * (cam.fx * p.x)) * rz2;
            gpz = gpz - (g[1] * (cam.fy * p.y)) * rz2;
            gpz = gpz + (clx ? limx * gtx : 0.0f);
            gpz = gpz + (cly ? limy * gty : 0.0f);
            // the unit direction d = v / |v| -> v: (gd - d (d . gd)) / |v|
            const float dg = (d[0] * gd[0] + d[1] * gd[1]) + d[2] * gd[2];
            const float wx = il * (gd[0] - d[0] * dg), wy = il * (gd[1] - d[1] * dg), wz = il * (gd[2] - d[2] * dg);
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

// What the three entries share: the model, the camera, the image size, where the statistics go and the stream.
struct RasterArgs {
    int64_t n;
    int32_t K, sh_degree;
    const float *xyz, *cov6, *raw_opacity, *dc, *sh_rest, *viewmat;
    float fx, fy, cx, cy;
    int32_t width, height;
    const float* background;
    float radius_clip;
    int64_t* stats_out;
    void* stream;
};

// What a render writes (device pointers or NULL).  rgb_only: gsr_raster_render, the image alone and required.
struct RasterForward {
    bool rgb_only;
    float *image, *depth, *alpha;
    uint32_t* contribution;
};

// What gsr_raster_backward adds to the arguments of a render: the two incoming gradients and the five outputs (device pointers or NULL).
struct RasterBackward {
    const float *grad_image, *grad_alpha;
    float *g_xyz, *g_cov6, *g_raw_opacity, *g_dc, *g_sh_rest;
};

// The render entries and the backward pass: validation (messages under the caller's name `who`), camera set-up, preprocess, sort, tile
// ranges, then the mode of k_raster_blend the outputs ask for (`fw`) or, with `bw`, k_raster_blend_bwd and k_raster_splat_bwd (timed by
// the context's second set of events).
static int32_t raster_run(const char* who, gsr_raster_ctx* c, const RasterArgs& a, const RasterForward& fw, const RasterBackward* bw = nullptr) {
    const int64_t n = a.n;
    const int32_t K = a.K, sh_degree = a.sh_degree, width = a.width, height = a.height;
    const bool rgb_only = fw.rgb_only;
    if (!c) return fail(GSR_E_INVALID, "%s: NULL context", who);
    if (n < 0 || n >= ((int64_t)1 << 31) - 1) return fail(GSR_E_INVALID, "%s: n = %lld out of range", who, (long long)n);
    if (sh_degree < 0 || sh_degree > 3 || K < (sh_degree + 1) * (sh_degree + 1) - 1)
        return fail(GSR_E_INVALID, "%s: sh_degree %d needs %d rest coefficients, K = %d", who, sh_degree, (sh_degree + 1) * (sh_degree + 1) - 1, K);
    if (width <= 0 || height <= 0 || width > 16 * 65535 || height > 16 * 65535) return fail(GSR_E_INVALID, "%s: bad image size %d x %d", who, width, height);
    if (!bw && !rgb_only && !fw.image && !fw.depth && !fw.alpha && !fw.contribution) return fail(GSR_E_INVALID, "%s: no output requested", who);
    if (bw && !bw->grad_image && !bw->grad_alpha) return fail(GSR_E_INVALID, "%s: grad_image and grad_alpha are both NULL", who);
    if (bw && !bw->g_xyz && !bw->g_cov6 && !bw->g_raw_opacity && !bw->g_dc && !bw->g_sh_rest) return fail(GSR_E_INVALID, "%s: no output requested", who);
    if (!a.viewmat || ((rgb_only || fw.image || (bw && bw->grad_image)) && !a.background) || (rgb_only && !fw.image) || !(a.fx > 0.0f) || !(a.fy > 0.0f))
        return fail(GSR_E_INVALID, "%s: NULL argument or focal length <= 0", who);
    if (n > 0 && (!a.xyz || !a.cov6 || !a.raw_opacity || !a.dc || (sh_degree > 0 && !a.sh_rest))) return fail(GSR_E_INVALID, "%s: NULL array", who);
    GSR_HIP(hipSetDevice(c->device));
    hipStream_t st = a.stream ? (hipStream_t)a.stream : c->stream;
    Event* ev = bw ? c->evb : c->ev;
    (bw ? c->timed_bwd : c->timed) = false;

    RasterCam cam;
    memset(&cam, 0, sizeof(cam));
    for (int r = 0; r < 3; ++r) {
        for (int q = 0; q < 3; ++q) cam.R[3 * r + q] = a.viewmat[4 * r + q];
        cam.t[r] = a.viewmat[4 * r + 3];
    }
    for (int q = 0; q < 3; ++q)          // camera position = -R^T t, float64 from the float32 matrix, narrowed once
        cam.cam[q] = (float)-((double)cam.R[q] * cam.t[0] + (double)cam.R[3 + q] * cam.t[1] + (double)cam.R[6 + q] * cam.t[2]);
    cam.fx = a.fx; cam.fy = a.fy; cam.cx = a.cx; cam.cy = a.cy;
    const float tan_x = 0.5f * (float)width / a.fx, tan_y = 0.5f * (float)height / a.fy;
    cam.lim_xp = ((float)width - a.cx) / a.fx + 0.3f * tan_x;
    cam.lim_xn = a.cx / a.fx + 0.3f * tan_x;
    cam.lim_yp = ((float)height - a.cy) / a.fy + 0.3f * tan_y;
    cam.lim_yn = a.cy / a.fy + 0.3f * tan_y;
    cam.near_z = 0.01f; cam.far_z = 1e10f; cam.eps2d = 0.3f; cam.radius_clip = a.radius_clip;
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
        hipLaunchKernelGGL(k_raster_preprocess, dim3(stride_grid(n)), dim3(256), 0, st, n, cam, a.xyz, a.cov6, a.raw_opacity, a.dc, a.sh_rest, c->splat.as<float>(),
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
        // what the sort (and the backward pass's records) still have to allocate, against what the device has free: an error with the
        // count, not an abort.  A buffer that must grow is freed first, so its capacity is given back.
        struct Sized { DevBuf& buf; size_t bytes; };
        const Sized sized[] = {{c->keys, ut * 8}, {c->keys2, ut * 8}, {c->vals, ut * 4}, {c->vals2, ut * 4}, {c->tmp, sort_bytes},
                               {c->rec, bw ? ut * SPLAT_WORDS * sizeof(float) : 0}};
        size_t need = 0, given_back = 0;
        for (const Sized& s : sized)
            if (s.bytes > s.buf.cap) { need += s.bytes + s.bytes / 8 + 256; given_back += s.buf.cap; }
        size_t free_b = 0, total_b = 0;
        GSR_HIP(hipMemGetInfo(&free_b, &total_b));
        if (need > free_b + given_back)
            return fail(GSR_E_HIP, "%s: %lld splat-tile intersections need %zu more bytes of %s, the device has %zu free", who, (long long)total, need,
                        bw ? "sort and gradient-record buffers" : "sort buffers", free_b + given_back);
        for (const Sized& s : sized) GSR_TRY(s.buf.reserve(s.bytes));
        hipLaunchKernelGGL(k_raster_emit, dim3(stride_grid(n)), dim3(256), 0, st, n, cam.tiles_x, c->depth.as<float>(), c->rect.as<ushort4>(), c->counts.as<int64_t>(),
                           c->offsets.as<int64_t>(), total, c->keys.as<uint64_t>(), c->vals.as<uint32_t>());
        GSR_HIP(rocprim::radix_sort_pairs(c->tmp.p, sort_bytes, c->keys.as<uint64_t>(), c->keys2.as<uint64_t>(), c->vals.as<uint32_t>(), c->vals2.as<uint32_t>(), ut,
                                          0u, end_bit, st));
        hipLaunchKernelGGL(k_raster_ranges, dim3(stride_grid(total)), dim3(256), 0, st, total, (int32_t)n_tiles, c->keys2.as<uint64_t>(), c->ranges.as<int64_t>(), counters);
    }
    GSR_HIP(hipEventRecord(ev[2], st));
    const dim3 tiles(cam.tiles_x, cam.tiles_y);
    const float bg[3] = {a.background ? a.background[0] : 0.0f, a.background ? a.background[1] : 0.0f, a.background ? a.background[2] : 0.0f};
    if (bw) {
        if (total > 0)
            hipLaunchKernelGGL(k_raster_blend_bwd, tiles, dim3(BLEND_THREADS), 0, st, width, height, cam.tiles_x, bg[0], bg[1], bg[2], n, c->ranges.as<int64_t>(),
                               c->vals2.as<uint32_t>(), c->splat.as<float>(), c->rect.as<ushort4>(), c->offsets.as<int64_t>(), total, bw->grad_image,
                               bw->grad_alpha, c->rec.as<float>());
        GSR_HIP(hipEventRecord(ev[3], st));
        if (n > 0)
            hipLaunchKernelGGL(k_raster_splat_bwd, dim3(stride_grid(n)), dim3(256), 0, st, n, cam, a.xyz, a.cov6, a.sh_rest, c->splat.as<float>(),
                               c->counts.as<int64_t>(), c->offsets.as<int64_t>(), c->rec.as<float>(), bw->g_xyz, bw->g_cov6, bw->g_raw_opacity, bw->g_dc,
                               bw->g_sh_rest);
        GSR_HIP(hipEventRecord(ev[4], st));
    } else {
        const auto blend = rgb_only ? k_raster_blend<BLEND_RGB> : fw.contribution ? k_raster_blend<BLEND_AUX_CONTRIB> : k_raster_blend<BLEND_AUX>;
        hipLaunchKernelGGL(blend, tiles, dim3(BLEND_THREADS), 0, st, width, height, cam.tiles_x, bg[0], bg[1], bg[2], n, c->ranges.as<int64_t>(),
                           c->vals2.as<uint32_t>(), c->splat.as<float>(), c->depth.as<float>(), fw.image, fw.depth, fw.alpha, fw.contribution);
        GSR_HIP(hipEventRecord(ev[3], st));
    }
    if (a.stats_out) GSR_HIP(hipMemcpyAsync(a.stats_out, counters, 3 * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    GSR_HIP(hipGetLastError());
    (bw ? c->timed_bwd : c->timed) = true;
    return GSR_OK;
}

extern "C" int32_t gsr_raster_render(gsr_raster_ctx* c, int64_t n, int32_t K, int32_t sh_degree, const float* xyz, const float* cov6, const float* raw_opacity,
                                     const float* dc, const float* sh_rest, const float* viewmat, float fx, float fy, float cx, float cy, int32_t width,
                                     int32_t height, const float* background, float radius_clip, float* image_out, int64_t* stats_out, void* stream) {
    const RasterArgs a = {n, K, sh_degree, xyz, cov6, raw_opacity, dc, sh_rest, viewmat, fx, fy, cx, cy, width, height, background, radius_clip, stats_out, stream};
    return raster_run("gsr_raster_render", c, a, {true, image_out, nullptr, nullptr, nullptr});
}

extern "C" int32_t gsr_raster_render_aux(gsr_raster_ctx* c, int64_t n, int32_t K, int32_t sh_degree, const float* xyz, const float* cov6, const float* raw_opacity,
                                         const float* dc, const float* sh_rest, const float* viewmat, float fx, float fy, float cx, float cy, int32_t width,
                                         int32_t height, const float* background, float radius_clip, float* image_out, float* depth_out, float* alpha_out,
                                         uint32_t* contribution_inout, int64_t* stats_out, void* stream) {
    const RasterArgs a = {n, K, sh_degree, xyz, cov6, raw_opacity, dc, sh_rest, viewmat, fx, fy, cx, cy, width, height, background, radius_clip, stats_out, stream};
    return raster_run("gsr_raster_render_aux", c, a, {false, image_out, depth_out, alpha_out, contribution_inout});
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
    const RasterArgs a = {n, K, sh_degree, xyz, cov6, raw_opacity, dc, sh_rest, viewmat, fx, fy, cx, cy, width, height, background, radius_clip, stats_out, stream};
    const RasterBackward bw = {grad_image, grad_alpha, grad_xyz, grad_cov6, grad_raw_opacity, grad_dc, grad_sh_rest};
    return raster_run("gsr_raster_backward", c, a, {false, nullptr, nullptr, nullptr, nullptr}, &bw);
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

constexpr int MT = 16, WIN = SSIM_WIN, HALO = 5, MTH = MT + 2 * HALO;       // 16 x 16 pixels per group, 26 x 26 with the halo

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
    const SsimWindow win = ssim_window();
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
