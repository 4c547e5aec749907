// warp.hip -- non-rigid refinement: a trilinear lattice of node displacements U that absorbs the smooth drift a
// single matrix leaves between two scenes.  Definitions (lattice, field, energy): include/gsr_hip.h; restated in float64 in
// tests/warp_model.py.  The solver is host code (gsr_warp.h); this file holds the device side:
//   gsr_warp_create / set_target / set_source   a context owning the target's point grid (GridIndex) with its normals, and the source
//   gsr_warp_accumulate      k_warp_match: a thread per source point -- cell and weights from the UNWARPED point, nearest target
//                            point of p + d(p) (expanding rings, strict d^2 < max_corr^2, lowest index on a tie); key = lattice cell
//                            rocPRIM radix sort of (cell, source index): stable, so a cell's matches stay in source order
//                            k_warp_plan: cell starts, and the first chunk of every cell (a chunk = 1024 consecutive matches of ONE cell)
//                            k_warp_gram: a wave per chunk; 64 points at a time put v = (g[24], r0, 1, 0) into LDS and a lane owns a
//                                         3 x 3 tile of the products v_a v_b, adding the chunk's points in order
//                            k_warp_fold: a thread per sum adds the cell's chunks in order
//                            No float atomics; the order of every sum is fixed by the data alone (source order inside a chunk, chunk
//                            order inside a cell), not by the launch.
//   gsr_warp_points          xyz -> float32(xyz + d(xyz))
//   gsr_model_warp           xyz and cov6 of a model: cov' = F cov F', F = I + sum U_k grad w_k'; counts det F <= 0
#include "gsr_common.h"
#include "gsr_grid.h"
#include "gsr_oneshot.h"
#include "gsr_prims.h"
#include "gsr_warp.h"

namespace gsr {

#define WARP_CHUNK 1024
#define WARP_VLEN 27          // g[24], r0, 1, 0
constexpr int WARP_CELL_LEN = warp::CELL_LEN;

struct Lattice {
    double lo[3], h[3];
    int n[3];
    int ncells;
};

// cell and weights of a point (float64): c_a = min(floor(clamp(s_a)), n_a - 2), f_a = clamp(s_a) - c_a; inv[a] = 1 / h_a where
// 0 < s_a < n_a - 1 strictly, else 0 (a clamped coordinate, or one on the outer face, has no derivative)
__device__ __forceinline__ void lattice_locate(const Lattice& L, const double p[3], int c[3], double f[3], double inv[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double top = (double)(L.n[a] - 1);
        const double s = (p[a] - L.lo[a]) / L.h[a];
        const double sb = fmin(fmax(s, 0.0), top);
        int ci = (int)floor(sb);
        ci = ci < L.n[a] - 2 ? ci : L.n[a] - 2;
        c[a] = ci;
        f[a] = sb - (double)ci;
        inv[a] = (s > 0.0 && s < top) ? 1.0 / L.h[a] : 0.0;
    }
}
__device__ __forceinline__ int lattice_cell(const Lattice& L, const int c[3]) { return (c[0] * (L.n[1] - 1) + c[1]) * (L.n[2] - 1) + c[2]; }
__device__ __forceinline__ int lattice_node(const Lattice& L, const int c[3], int k) {
    return ((c[0] + (k >> 2)) * L.n[1] + c[1] + ((k >> 1) & 1)) * L.n[2] + c[2] + (k & 1);
}
// w_k = (X Y) Z, local node k = 4 bx + 2 by + bz
__device__ __forceinline__ void lattice_weights(const double f[3], double w[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const double X = (k & 4) ? f[0] : 1.0 - f[0], Y = (k & 2) ? f[1] : 1.0 - f[1], Z = (k & 1) ? f[2] : 1.0 - f[2];
        w[k] = (X * Y) * Z;
    }
}
// d(p) = sum_k w_k U_k, k ascending
__device__ __forceinline__ void lattice_displace(const Lattice& L, const double* __restrict__ U, const int c[3], const double w[8], double d[3]) {
    d[0] = d[1] = d[2] = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const double* u = U + 3 * (int64_t)lattice_node(L, c, k);
        d[0] += w[k] * u[0]; d[1] += w[k] * u[1]; d[2] += w[k] * u[2];
    }
}

// Exact nearest target point of p with d^2 < bound2, lowest input index on a tie: the ring loop of the ICP search (csrc/icp.hip,
// icp_nearest<0>) -- rows pruned by the best so far, strictly, so that a point at exactly the best distance can still win its tie.
__device__ __forceinline__ int warp_nearest(const IcpGrid& g, const int* __restrict__ cellStart, const float4* __restrict__ Tq, double px, double py, double pz,
                                            double bound2) {
    int best = -1;
    unsigned best_i = 0xffffffffu;
    double bd = bound2;
    {
        const double ex = fmax(fmax(g.bx0 - px, px - g.bx1), 0.0), ey = fmax(fmax(g.by0 - py, py - g.by1), 0.0), ez = fmax(fmax(g.bz0 - pz, pz - g.bz1), 0.0);
        if ((ex * ex + ey * ey + ez * ez) * 0.999999999 >= bound2) return -1;
    }
    const int cx = icp_cell(px, g.ox, g.inv_c, g.gx), cy = icp_cell(py, g.oy, g.inv_c, g.gy), cz = icp_cell(pz, g.oz, g.inv_c, g.gz);
    const double eps = 1e-13 * (fabs(px) + fabs(py) + fabs(pz) + fabs(g.ox) + fabs(g.oy) + fabs(g.oz) + g.c * (double)(g.gx + g.gy + g.gz));
    auto scan = [&](int first, int last) {
        const int s = cellStart[first], e = cellStart[last + 1];
        for (int j = s; j < e; ++j) {
            const float4 q = Tq[j];
            const double dx = px - (double)q.x, dy = py - (double)q.y, dz = pz - (double)q.z;
            const double d2 = dx * dx + dy * dy + dz * dz;
            const unsigned qi = __float_as_uint(q.w);
            if (d2 < bd || (d2 == bd && best >= 0 && qi < best_i)) { bd = d2; best = j; best_i = qi; }
        }
    };
    for (int r = 0; r <= g.rings; ++r) {
        for (int dz = -r; dz <= r; ++dz) {
            const int z = cz + dz;
            if (z < 0 || z >= g.gz) continue;
            const int adz = dz < 0 ? -dz : dz;
            const double dzb = icp_slab_dist(pz, g.oz, g.c, z, eps, g.gz);
            for (int dy = -r; dy <= r; ++dy) {
                const int y = cy + dy;
                if (y < 0 || y >= g.gy) continue;
                const int ady = dy < 0 ? -dy : dy;
                const double dyb = icp_slab_dist(py, g.oy, g.c, y, eps, g.gy);
                const double rem = bd - dyb * dyb - dzb * dzb;
                if (rem < 0.0) continue;
                const double hx = (double)(sqrtf((float)rem) * 1.0001f) + eps + 1e-30;
                const int xlo = icp_cell(px - hx, g.ox, g.inv_c, g.gx), xhi = icp_cell(px + hx, g.ox, g.inv_c, g.gx);
                const int rowbase = (z * g.gy + y) * g.gx;
                if (adz == r || ady == r) {
                    int xa = cx - r > 0 ? cx - r : 0, xb = cx + r < g.gx - 1 ? cx + r : g.gx - 1;
                    xa = xa > xlo ? xa : xlo;
                    xb = xb < xhi ? xb : xhi;
                    if (xa <= xb) scan(rowbase + xa, rowbase + xb);
                } else {
                    if (cx - r >= 0 && cx - r >= xlo) scan(rowbase + cx - r, rowbase + cx - r);
                    if (cx + r < g.gx && cx + r <= xhi) scan(rowbase + cx + r, rowbase + cx + r);
                }
            }
        }
        double reach = 1.0 / 0.0;
        if (cx - r > 0) reach = fmin(reach, px - (g.ox + (double)(cx - r) * g.c));
        if (cx + r < g.gx - 1) reach = fmin(reach, (g.ox + (double)(cx + r + 1) * g.c) - px);
        if (cy - r > 0) reach = fmin(reach, py - (g.oy + (double)(cy - r) * g.c));
        if (cy + r < g.gy - 1) reach = fmin(reach, (g.oy + (double)(cy + r + 1) * g.c) - py);
        if (cz - r > 0) reach = fmin(reach, pz - (g.oz + (double)(cz - r) * g.c));
        if (cz + r < g.gz - 1) reach = fmin(reach, (g.oz + (double)(cz + r + 1) * g.c) - pz);
        reach = reach * 0.999999999 - eps;
        reach = reach > 0.0 ? reach : 0.0;
        if (bd < reach * reach) break;
    }
    return best;
}

// key[i] = lattice cell of source point i when it has a correspondence, else ncells; nn[i] = sorted position of its target point
__global__ __launch_bounds__(256) void k_warp_match(int64_t ns, const float* __restrict__ src, Lattice L, const double* __restrict__ U, IcpGrid g,
                                                    const int* __restrict__ cellStart, const float4* __restrict__ Tq, double max_corr2,
                                                    unsigned* __restrict__ key, unsigned* __restrict__ idx, int* __restrict__ nn) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ns; i += (int64_t)gridDim.x * blockDim.x) {
        const double p[3] = {(double)src[3 * i], (double)src[3 * i + 1], (double)src[3 * i + 2]};
        unsigned k = (unsigned)L.ncells;
        int j = -1;
        if (isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])) {
            int c[3];
            double f[3], inv[3], w[8], d[3];
            lattice_locate(L, p, c, f, inv);
            lattice_weights(f, w);
            lattice_displace(L, U, c, w, d);
            j = warp_nearest(g, cellStart, Tq, p[0] + d[0], p[1] + d[1], p[2] + d[2], max_corr2);
            if (j >= 0) k = (unsigned)lattice_cell(L, c);
        }
        key[i] = k;
        idx[i] = (unsigned)i;
        nn[i] = j;
    }
}

// cellStart[c] = first sorted entry with key >= c (c = 0 .. ncells: the last one is the number of correspondences);
// chunkBase[c] = chunks of the cells before c.  One workgroup.
__global__ __launch_bounds__(256) void k_warp_plan(int64_t ns, int ncells, const unsigned* __restrict__ skey, int* __restrict__ cellStart, int* __restrict__ chunkBase) {
    for (int c = threadIdx.x; c <= ncells; c += blockDim.x) {
        int64_t lo = 0, hi = ns;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (skey[mid] < (unsigned)c) lo = mid + 1; else hi = mid;
        }
        cellStart[c] = (int)lo;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int base = 0;
        for (int c = 0; c < ncells; ++c) {
            chunkBase[c] = base;
            base += (cellStart[c + 1] - cellStart[c] + WARP_CHUNK - 1) / WARP_CHUNK;
        }
        chunkBase[ncells] = base;
    }
}

// One wave per chunk.  326 running sums do not fit a lane (652 VGPRs), so the wave holds them together: v v' (27 x 27 with the zero
// slot) is cut into 3 x 3 tiles, the 45 tiles on or above the diagonal go to lanes 0..44, and a lane keeps its tile's nine sums.  The
// points' vectors go through LDS, 64 at a time; per point a lane reads the six values of its tile's rows and columns (a first
// version gave every lane six scattered products, twelve reads per point: the kernel is bound by those reads and took twice as long,
// DESIGN.md 24).  Every sum adds its chunk's points in order, whatever the layout.
__global__ __launch_bounds__(64) void k_warp_gram(const float* __restrict__ src, Lattice L, const unsigned* __restrict__ sidx, const int* __restrict__ nn,
                                                  const float4* __restrict__ Tq, const double* __restrict__ Tn, const int* __restrict__ cellStart,
                                                  const int* __restrict__ chunkBase, double* __restrict__ partials) {
    __shared__ double sv[64][WARP_VLEN];
    const int lane = threadIdx.x, chunk = blockIdx.x;
    if (chunk >= chunkBase[L.ncells]) return;
    int lo = 0, hi = L.ncells;                          // the cell: the last c with chunkBase[c] <= chunk that has chunks
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (chunkBase[mid] <= chunk) lo = mid; else hi = mid;
    }
    const int cell = lo;
    const int start = cellStart[cell] + (chunk - chunkBase[cell]) * WARP_CHUNK;
    const int end = start + WARP_CHUNK < cellStart[cell + 1] ? start + WARP_CHUNK : cellStart[cell + 1];
    int ti = 0, tj = 0;                                 // the lane's tile: rows 3 ti .., columns 3 tj .., ti <= tj < 9 (lanes 45..63 idle along tile 44)
    {
        int t = lane < 45 ? lane : 44;
        while (t >= 9 - ti) { t -= 9 - ti; ++ti; }
        tj = ti + t;
    }
    double acc[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    for (int base = start; base < end; base += 64) {
        const int at = base + lane;
        if (at < end) {
            const int64_t i = (int64_t)sidx[at];
            const double p[3] = {(double)src[3 * i], (double)src[3 * i + 1], (double)src[3 * i + 2]};
            int c[3];
            double f[3], inv[3], w[8];
            lattice_locate(L, p, c, f, inv);
            lattice_weights(f, w);
            const int j = nn[i];
            const float4 q = Tq[j];
            const double nx = Tn[3 * (int64_t)j], ny = Tn[3 * (int64_t)j + 1], nz = Tn[3 * (int64_t)j + 2];
            const double r0 = (p[0] - (double)q.x) * nx + (p[1] - (double)q.y) * ny + (p[2] - (double)q.z) * nz;
#pragma unroll
            for (int k = 0; k < 8; ++k) { sv[lane][3 * k] = w[k] * nx; sv[lane][3 * k + 1] = w[k] * ny; sv[lane][3 * k + 2] = w[k] * nz; }
            sv[lane][24] = r0; sv[lane][25] = 1.0; sv[lane][26] = 0.0;
        }
        __syncthreads();
        const int cnt = end - base < 64 ? end - base : 64;
        for (int m = 0; m < cnt; ++m) {
            const double a0 = sv[m][3 * ti], a1 = sv[m][3 * ti + 1], a2 = sv[m][3 * ti + 2];
            const double b0 = sv[m][3 * tj], b1 = sv[m][3 * tj + 1], b2 = sv[m][3 * tj + 2];
            acc[0][0] += a0 * b0; acc[0][1] += a0 * b1; acc[0][2] += a0 * b2;
            acc[1][0] += a1 * b0; acc[1][1] += a1 * b1; acc[1][2] += a1 * b2;
            acc[2][0] += a2 * b0; acc[2][1] += a2 * b1; acc[2][2] += a2 * b2;
        }
        __syncthreads();
    }
    if (lane >= 45) return;
    double* out = partials + (int64_t)chunk * WARP_CELL_LEN;
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
        for (int y = 0; y < 3; ++y) {
            const int a = 3 * ti + x, b = 3 * tj + y;       // the product v_a v_b; kept where it is one of the 326
            if (a > b) continue;
            if (b < 24) out[a * 24 - a * (a - 1) / 2 + (b - a)] = acc[x][y];
            else if (b == 24) out[a < 24 ? 300 + a : 324] = acc[x][y];
            else if (a == 25 && b == 25) out[325] = acc[x][y];
        }
}

__global__ __launch_bounds__(384) void k_warp_fold(const int* __restrict__ chunkBase, const double* __restrict__ partials, double* __restrict__ sums) {
    const int cell = blockIdx.x, e = threadIdx.x;
    if (e >= WARP_CELL_LEN) return;
    double s = 0.0;
    for (int g = chunkBase[cell]; g < chunkBase[cell + 1]; ++g) s += partials[(int64_t)g * WARP_CELL_LEN + e];
    sums[(int64_t)cell * WARP_CELL_LEN + e] = s;
}

__global__ __launch_bounds__(256) void k_warp_points(int64_t n, Lattice L, const double* __restrict__ U, const float* __restrict__ xyz, float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float x[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
        float o[3] = {x[0], x[1], x[2]};
        const double p[3] = {(double)x[0], (double)x[1], (double)x[2]};
        if (isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])) {
            int c[3];
            double f[3], inv[3], w[8], d[3];
            lattice_locate(L, p, c, f, inv);
            lattice_weights(f, w);
            lattice_displace(L, U, c, w, d);
            o[0] = (float)(p[0] + d[0]); o[1] = (float)(p[1] + d[1]); o[2] = (float)(p[2] + d[2]);
        }
        out[3 * i] = o[0]; out[3 * i + 1] = o[1]; out[3 * i + 2] = o[2];
    }
}

// xyz' = float32(p + d(p)); cov' = F cov F' in float64, rounded once; a row with a non-finite coordinate is copied.  *folded counts
// the finite rows with det F <= 0 (an integer atomic per wave).
__global__ __launch_bounds__(256) void k_model_warp(int64_t n, Lattice L, const double* __restrict__ U, const float* __restrict__ xyz, const float* __restrict__ cov6,
                                                    float* __restrict__ xyz_out, float* __restrict__ cov_out, unsigned long long* __restrict__ folded) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t n_up = (n + 63) / 64 * 64;            // whole waves take every trip (wave_count)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_up; i += stride) {
        bool fold = false;
        if (i < n) {
            const float x[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
            float o[3] = {x[0], x[1], x[2]};
            float S[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) S[k] = cov6[6 * i + k];
            const double p[3] = {(double)x[0], (double)x[1], (double)x[2]};
            if (isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])) {
                int c[3];
                double f[3], inv[3], w[8];
                lattice_locate(L, p, c, f, inv);
                lattice_weights(f, w);
                double d[3] = {0.0, 0.0, 0.0}, J[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const double X = (k & 4) ? f[0] : 1.0 - f[0], Y = (k & 2) ? f[1] : 1.0 - f[1], Z = (k & 1) ? f[2] : 1.0 - f[2];
                    const double gw[3] = {(((k & 4) ? inv[0] : -inv[0]) * Y) * Z, (X * ((k & 2) ? inv[1] : -inv[1])) * Z, (X * Y) * ((k & 1) ? inv[2] : -inv[2])};
                    const double* u = U + 3 * (int64_t)lattice_node(L, c, k);
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        d[a] += w[k] * u[a];
#pragma unroll
                        for (int b = 0; b < 3; ++b) J[a][b] += u[a] * gw[b];
                    }
                }
                double F[3][3];
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int b = 0; b < 3; ++b) F[a][b] = (a == b ? 1.0 : 0.0) + J[a][b];
                const double det = (F[0][0] * (F[1][1] * F[2][2] - F[1][2] * F[2][1]) - F[0][1] * (F[1][0] * F[2][2] - F[1][2] * F[2][0])) +
                                   F[0][2] * (F[1][0] * F[2][1] - F[1][1] * F[2][0]);
                fold = det <= 0.0;
                const double C[3][3] = {{(double)S[0], (double)S[1], (double)S[2]}, {(double)S[1], (double)S[3], (double)S[4]}, {(double)S[2], (double)S[4], (double)S[5]}};
                double Mx[3][3];
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int b = 0; b < 3; ++b) Mx[a][b] = (F[a][0] * C[0][b] + F[a][1] * C[1][b]) + F[a][2] * C[2][b];
                int t = 0;
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int b = a; b < 3; ++b) S[t++] = (float)((Mx[a][0] * F[b][0] + Mx[a][1] * F[b][1]) + Mx[a][2] * F[b][2]);
                o[0] = (float)(p[0] + d[0]); o[1] = (float)(p[1] + d[1]); o[2] = (float)(p[2] + d[2]);
            }
            xyz_out[3 * i] = o[0]; xyz_out[3 * i + 1] = o[1]; xyz_out[3 * i + 2] = o[2];
#pragma unroll
            for (int k = 0; k < 6; ++k) cov_out[6 * i + k] = S[k];
        }
        wave_count(fold, folded);
    }
}

// the lattice of a call, checked: "" or why not
static std::string make_lattice(const double* lo, const double* hi, const int32_t* dims, const double* U, Lattice* L, bool* flat) {
    char msg[160];
    if (!lo || !hi || !dims || !U) return "NULL lattice argument";
    if (!warp::dims_ok(dims)) { snprintf(msg, sizeof msg, "lattice dimensions (%d, %d, %d) outside [2, 17]", dims[0], dims[1], dims[2]); return msg; }
    for (int a = 0; a < 3; ++a) {
        if (!isfinite(lo[a]) || !isfinite(hi[a]) || !(hi[a] > lo[a])) { snprintf(msg, sizeof msg, "lattice box: axis %d is [%g, %g]", a, lo[a], hi[a]); return msg; }
        L->lo[a] = lo[a];
        L->h[a] = (hi[a] - lo[a]) / (double)(dims[a] - 1);
        L->n[a] = dims[a];
        if (!(L->h[a] > 0) || !isfinite(L->h[a])) { snprintf(msg, sizeof msg, "lattice box: axis %d has no extent", a); return msg; }
    }
    L->ncells = warp::n_cells(dims);
    bool zero = true;
    for (int i = 0; i < 3 * warp::n_nodes(dims); ++i) {
        if (!isfinite(U[i])) { snprintf(msg, sizeof msg, "non-finite displacement (node %d)", i / 3); return msg; }
        zero = zero && U[i] == 0.0;
    }
    *flat = zero;
    return "";
}

// U = 0: the rows as they are, on the side they live on
static int32_t copy_rows(OneShot& os, float* out, const float* in, size_t bytes) {
    if (out == in) return GSR_OK;
    if (os.on_device) GSR_HIP(hipMemcpyAsync(out, in, bytes, hipMemcpyDeviceToDevice, os.st));
    else memmove(out, in, bytes);
    return GSR_OK;
}

}  // namespace gsr

using namespace gsr;

struct gsr_warp_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    GridIndex index;                // the target's point grid (gsr_grid.h)
    DevBuf Tn, stage_xyz, stage_nrm, src, U, key, idx, skey, sidx, nn, cellStart, chunkBase, partials, sums, rocprim_tmp;
    bool have_target = false, have_source = false;
    int64_t nt = 0, ns = 0;
    double max_corr = 0;
    ~gsr_warp_ctx() { (void)hipSetDevice(device); }
};

extern "C" {

int32_t gsr_warp_create(gsr_warp_ctx** out, int32_t device, void* stream) {
    if (!out) return fail(GSR_E_INVALID, "gsr_warp_create: out is NULL");
    *out = nullptr;
    GSR_TRY(open_device(device, "gsr_warp_create"));
    gsr_warp_ctx* c = new gsr_warp_ctx();
    c->device = device;
    c->stream = (hipStream_t)stream;
    *out = c;
    return GSR_OK;
}

int32_t gsr_warp_destroy(gsr_warp_ctx* c) {
    delete c;       // (NULL: nothing)
    return GSR_OK;
}

int32_t gsr_warp_set_target(gsr_warp_ctx* c, const float* xyz, const double* normals, int64_t n, double max_corr, int32_t on_device) {
    if (!c) return fail(GSR_E_INVALID, "gsr_warp_set_target: NULL context");
    if (!(max_corr > 0) || !isfinite(max_corr)) return fail(GSR_E_INVALID, "gsr_warp_set_target: max_corr must be positive and finite (got %g)", max_corr);
    if (n <= 0 || !xyz || !normals) return fail(GSR_E_INVALID, "gsr_warp_set_target: the target needs points and normals");
    if (n >= ((int64_t)1 << 31) - 1) return fail(GSR_E_INVALID, "gsr_warp_set_target: n too large");
    GSR_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    c->have_target = false;
    const float* dxyz = xyz;
    const double* dnrm = normals;
    if (!on_device) {
        GSR_TRY(c->stage_xyz.reserve((size_t)n * 12));
        GSR_TRY(c->stage_nrm.reserve((size_t)n * 24));
        GSR_HIP(hipMemcpyAsync(c->stage_xyz.p, xyz, (size_t)n * 12, hipMemcpyHostToDevice, st));
        GSR_HIP(hipMemcpyAsync(c->stage_nrm.p, normals, (size_t)n * 24, hipMemcpyHostToDevice, st));
        dxyz = c->stage_xyz.as<float>();
        dnrm = c->stage_nrm.as<double>();
    }
    GSR_TRY(c->Tn.reserve((size_t)n * 24));
    GSR_TRY(c->index.build(dxyz, n, max_corr, st, dnrm, c->Tn.as<double>()));
    GSR_HIP(hipStreamSynchronize(st));
    c->nt = n;
    c->max_corr = max_corr;
    c->have_target = true;
    return GSR_OK;
}

int32_t gsr_warp_set_source(gsr_warp_ctx* c, const float* xyz, int64_t n, int32_t on_device) {
    if (!c) return fail(GSR_E_INVALID, "gsr_warp_set_source: NULL context");
    if (n < 0 || (n > 0 && !xyz)) return fail(GSR_E_INVALID, "gsr_warp_set_source: bad argument");
    if (n >= ((int64_t)1 << 31) - 1) return fail(GSR_E_INVALID, "gsr_warp_set_source: n too large");
    GSR_HIP(hipSetDevice(c->device));
    c->have_source = false;
    if (n > 0) {
        GSR_TRY(c->src.reserve((size_t)n * 12));
        GSR_HIP(hipMemcpyAsync(c->src.p, xyz, (size_t)n * 12, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
        GSR_HIP(hipStreamSynchronize(c->stream));
    }
    c->ns = n;
    c->have_source = true;
    return GSR_OK;
}

int32_t gsr_warp_accumulate(gsr_warp_ctx* c, const double* lo3, const double* hi3, const int32_t* dims3, const double* U, double* sums, int64_t* n_corr,
                            double* rmse) {
    if (!c) return fail(GSR_E_INVALID, "gsr_warp_accumulate: NULL context");
    if (!c->have_target || !c->have_source) return fail(GSR_E_INVALID, "gsr_warp_accumulate: target and source must be set first");
    if (!sums) return fail(GSR_E_INVALID, "gsr_warp_accumulate: sums is NULL");
    Lattice L;
    bool flat = false;
    const std::string err = make_lattice(lo3, hi3, dims3, U, &L, &flat);
    if (!err.empty()) return fail(GSR_E_INVALID, "gsr_warp_accumulate: %s", err.c_str());
    GSR_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int ncells = L.ncells, M = warp::n_nodes(dims3);
    const int64_t ns = c->ns;
    const size_t sums_bytes = (size_t)ncells * WARP_CELL_LEN * 8;
    if (ns == 0) memset(sums, 0, sums_bytes);
    else {
        const int64_t max_chunks = ns / WARP_CHUNK + ncells + 1;
        GSR_TRY(c->U.reserve((size_t)M * 24));
        GSR_TRY(c->key.reserve((size_t)ns * 4)); GSR_TRY(c->idx.reserve((size_t)ns * 4));
        GSR_TRY(c->skey.reserve((size_t)ns * 4)); GSR_TRY(c->sidx.reserve((size_t)ns * 4));
        GSR_TRY(c->nn.reserve((size_t)ns * 4));
        GSR_TRY(c->cellStart.reserve(((size_t)ncells + 1) * 4)); GSR_TRY(c->chunkBase.reserve(((size_t)ncells + 1) * 4));
        GSR_TRY(c->partials.reserve((size_t)max_chunks * WARP_CELL_LEN * 8));
        GSR_TRY(c->sums.reserve(sums_bytes));
        GSR_HIP(hipMemcpyAsync(c->U.p, U, (size_t)M * 24, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_warp_match, dim3(stride_grid(ns)), dim3(256), 0, st, ns, c->src.as<float>(), L, c->U.as<double>(), c->index.grid, c->index.cellStart.as<int>(),
                           c->index.Tq.as<float4>(), c->max_corr * c->max_corr, c->key.as<unsigned>(), c->idx.as<unsigned>(), c->nn.as<int>());
        unsigned bits = 1;
        while (bits < 32 && (1u << bits) <= (unsigned)ncells) ++bits;
        GSR_TRY((sort_pairs_by_key<rocprim::default_config>(c->rocprim_tmp, st, c->key.as<unsigned>(), c->skey.as<unsigned>(), c->idx.as<unsigned>(), c->sidx.as<unsigned>(),
                                                            (size_t)ns, 0u, bits)));
        hipLaunchKernelGGL(k_warp_plan, dim3(1), dim3(256), 0, st, ns, ncells, c->skey.as<unsigned>(), c->cellStart.as<int>(), c->chunkBase.as<int>());
        hipLaunchKernelGGL(k_warp_gram, dim3((unsigned)max_chunks), dim3(64), 0, st, c->src.as<float>(), L, c->sidx.as<unsigned>(), c->nn.as<int>(), c->index.Tq.as<float4>(),
                           c->Tn.as<double>(), c->cellStart.as<int>(), c->chunkBase.as<int>(), c->partials.as<double>());
        hipLaunchKernelGGL(k_warp_fold, dim3(ncells), dim3(384), 0, st, c->chunkBase.as<int>(), c->partials.as<double>(), c->sums.as<double>());
        GSR_HIP(hipGetLastError());
        GSR_HIP(hipMemcpyAsync(sums, c->sums.p, sums_bytes, hipMemcpyDeviceToHost, st));
        GSR_HIP(hipStreamSynchronize(st));
    }
    // the count and the RMSE at U from the sums: sum (r0 + g' U)^2 = S_rr + 2 b' u + u' A u per cell
    double nC = 0, ss = 0;
    for (int cell = 0; cell < ncells; ++cell) {
        const double* s = sums + (size_t)cell * WARP_CELL_LEN;
        if (s[325] == 0) continue;
        nC += s[325];
        int nd[8];
        warp::cell_nodes(dims3, cell, nd);
        double u[24], q = 0, l = 0;
        for (int k = 0; k < 8; ++k)
            for (int a = 0; a < 3; ++a) u[3 * k + a] = U[3 * nd[k] + a];
        for (int a = 0; a < 24; ++a) {
            l += s[300 + a] * u[a];
            q += s[warp::tri(a, a)] * u[a] * u[a];
            for (int b = a + 1; b < 24; ++b) q += 2.0 * s[warp::tri(a, b)] * u[a] * u[b];
        }
        ss += s[324] + 2.0 * l + q;
    }
    if (n_corr) *n_corr = (int64_t)nC;
    if (rmse) *rmse = nC > 0 ? sqrt(fmax(ss, 0.0) / nC) : 0.0;
    return GSR_OK;
}

int32_t gsr_warp_points(const double* lo3, const double* hi3, const int32_t* dims3, const double* U, const float* xyz, int64_t n, float* xyz_out,
                        int32_t on_device, int32_t device, void* stream) {
    if (n < 0 || (n > 0 && (!xyz || !xyz_out))) return fail(GSR_E_INVALID, "gsr_warp_points: bad argument");
    Lattice L;
    bool flat = false;
    const std::string err = make_lattice(lo3, hi3, dims3, U, &L, &flat);
    if (!err.empty()) return fail(GSR_E_INVALID, "gsr_warp_points: %s", err.c_str());
    GSR_TRY(open_device(device, "gsr_warp_points"));
    if (n == 0) return GSR_OK;
    OneShot os((hipStream_t)stream, on_device != 0, "gsr_warp_points");
    if (flat) {                                          // U = 0: the input's bits (p + 0.0 would turn a -0.0 into +0.0)
        GSR_TRY(copy_rows(os, xyz_out, xyz, (size_t)n * 12));
        return os.wait();
    }
    const float* dx = nullptr;
    const double* dU = nullptr;
    float* dout = nullptr;
    OneShot osU((hipStream_t)stream, false, "gsr_warp_points");      // U is on the host whatever the arrays are
    GSR_TRY(osU.in(U, (size_t)warp::n_nodes(dims3) * 24, &dU));
    GSR_TRY(os.in(xyz, (size_t)n * 12, &dx));
    GSR_TRY(os.out(xyz_out, (size_t)n * 12, &dout));
    hipLaunchKernelGGL(k_warp_points, dim3(stride_grid(n)), dim3(256), 0, os.st, n, L, dU, dx, dout);
    return os.finish();
}

int32_t gsr_model_warp(const double* lo3, const double* hi3, const int32_t* dims3, const double* U, int64_t n, const float* xyz, const float* cov6,
                       float* xyz_out, float* cov6_out, int64_t* n_folded, int32_t on_device, int32_t device, void* stream) {
    if (n < 0 || (n > 0 && (!xyz || !cov6 || !xyz_out || !cov6_out))) return fail(GSR_E_INVALID, "gsr_model_warp: bad argument");
    Lattice L;
    bool flat = false;
    const std::string err = make_lattice(lo3, hi3, dims3, U, &L, &flat);
    if (!err.empty()) return fail(GSR_E_INVALID, "gsr_model_warp: %s", err.c_str());
    GSR_TRY(open_device(device, "gsr_model_warp"));
    if (n_folded) *n_folded = 0;
    if (n == 0) return GSR_OK;
    unsigned long long folded_host = 0;                  // before the OneShots: their waits end before it leaves the frame
    OneShot os((hipStream_t)stream, on_device != 0, "gsr_model_warp");
    if (flat) {
        GSR_TRY(copy_rows(os, xyz_out, xyz, (size_t)n * 12));
        GSR_TRY(copy_rows(os, cov6_out, cov6, (size_t)n * 24));
        return os.wait();
    }
    OneShot osU((hipStream_t)stream, false, "gsr_model_warp");       // U and the counter: host memory whatever the arrays are
    const float *dx = nullptr, *dc = nullptr;
    const double* dU = nullptr;
    float *ox = nullptr, *oc = nullptr;
    unsigned long long* dfold = nullptr;
    GSR_TRY(osU.in(U, (size_t)warp::n_nodes(dims3) * 24, &dU));
    GSR_TRY(osU.out(&folded_host, 8, &dfold));
    GSR_TRY(os.in(xyz, (size_t)n * 12, &dx));
    GSR_TRY(os.in(cov6, (size_t)n * 24, &dc));
    GSR_TRY(os.out(xyz_out, (size_t)n * 12, &ox));
    GSR_TRY(os.out(cov6_out, (size_t)n * 24, &oc));
    GSR_HIP(hipMemsetAsync(dfold, 0, 8, os.st));
    hipLaunchKernelGGL(k_model_warp, dim3(stride_grid(n)), dim3(256), 0, os.st, n, L, dU, dx, dc, ox, oc, dfold);
    GSR_TRY(os.finish());
    GSR_TRY(osU.finish());
    if (n_folded) *n_folded = (int64_t)folded_host;
    return GSR_OK;
}

int32_t gsr_warp_solve(const int32_t* dims3, const double* sums, double lam, double lam0, double* U, gsr_warp_report* report) {
    warp::Report r;
    const std::string err = warp::solve(dims3, sums, lam, lam0, U, &r);
    if (!err.empty()) return fail(GSR_E_INVALID, "gsr_warp_solve: %s", err.c_str());
    if (report) {
        report->E_before = r.E_before; report->E_after = r.E_after;
        report->E_data_before = r.E_data_before; report->E_data_after = r.E_data_after;
        report->n_corr = r.n_corr;
        report->n_unknowns = r.n_unknowns; report->half_band = r.half_band;
        report->pivot_min = r.pivot_min; report->pivot_max = r.pivot_max;
    }
    return GSR_OK;
}

}  // extern "C"
