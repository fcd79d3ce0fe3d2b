// fields3d.hip -- the 3-D projection step around the 3-D pressure solves, for
// gfx950: fused advection-diffusion predictor, divergence, gradient +
// projection, lid-driven cavity walls, the cylinder channel's boundary
// conditions with the immersed-boundary forcing, the vorticity and the energy /
// clip epilogue on (nz, ny, nx) float32 fields u, v, w (x fastest; E/W = x+-1,
// N/S = y+-1, U/D = z+-1).
//
// The arithmetic is the project's own 3-D generalisation of the v5 templates
// (fields2d.hip), every 2-D coefficient kept and a z term appended to each
// sum; tests/ref3d.py states it as NumPy array code and the kernels reproduce
// it bit for bit (float32 operations in the source order, nothing fused).
// All indexing is 64-bit.
#include <map>
#include <mutex>
#include <type_traits>

#include "common.hpp"
#include "internal.hpp"
#include "pred_planes.hpp"

namespace cfd {

__device__ inline bool interior3(int k, int j, int i, int nz, int ny, int nx) {
    return k >= 1 && k < nz - 1 && j >= 1 && j < ny - 1 && i >= 1 && i < nx - 1;
}

// ZP (spanwise-periodic z, the *_zper entry points): every plane is interior
// in z, the U neighbour of plane nz - 1 is plane 0 and the D neighbour of plane
// 0 is plane nz - 1; the four x / y faces are what they were.  A template
// parameter of the per-cell kernels: ZP = false is the code it was.
template <bool ZP>
__device__ inline bool interior3z(int k, int j, int i, int nz, int ny, int nx) {
    return (ZP || (k >= 1 && k < nz - 1)) && j >= 1 && j < ny - 1 && i >= 1 && i < nx - 1;
}
// the U / D neighbours' indices (CFD_3D_INDEX's names; wrapped when ZP)
#define CFD_3D_UD(ZP)                                                                 \
    const size_t cu = (ZP) && k == nz - 1 ? c - (size_t)(nz - 1) * sz : c + sz;       \
    const size_t cd = (ZP) && k == 0 ? c + (size_t)(nz - 1) * sz : c - sz;

// one thread per cell: blockIdx.y = row, blockIdx.z = plane
#define CFD_3D_INDEX                                     \
    const int i = blockIdx.x * blockDim.x + threadIdx.x; \
    const int j = blockIdx.y;                            \
    const int k = blockIdx.z;                            \
    const bool cell = i < nx;                            \
    const size_t sy = (size_t)nx, sz = (size_t)ny * nx;  \
    const size_t c = ((size_t)k * ny + j) * nx + (cell ? i : 0);

// The fused predictor, one thread per cell (plain loads; the neighbours come
// from L1 / L2): the fallback of the plane march for unaligned shapes and its
// yardstick.  pred3_tau / pred3_cell / smag3_nut: pred_planes.hpp.  NM: the
// viscosity mode (kNu3Scalar: nu; kNu3Array: nu_arr per cell; kNu3Les:
// (nu + nu_t) + art with nu_t formed here and written to nut unless null).
struct Pred3Nu {
    const float *nu_arr;
    float *nut;
    float c2, art;
};
// the trailing mode arguments of k_predictor3d, picked by type
__device__ inline Pred3Nu pred3_mode_nu() { return {}; }
__device__ inline Pred3Nu pred3_mode_nu(const Pred3Nu &m) { return m; }
__device__ inline Pred3Nu pred3_mode_nu(const Pred3Buoy &) { return {}; }
__device__ inline Pred3Nu pred3_mode_nu(const Pred3Nu &m, const Pred3Buoy &) { return m; }
__device__ inline Pred3Buoy pred3_mode_buoy(const Pred3Buoy &b) { return b; }
__device__ inline Pred3Buoy pred3_mode_buoy(const Pred3Nu &, const Pred3Buoy &b) { return b; }
// M: one Pred3Nu for the array and LES modes, empty for the scalar one (whose
// argument list, and with it its code, stays what it was before the modes);
// then one Pred3Buoy for the buoyant form (scalar and LES only), which adds
// dt * (b_f * (T - t_ref)) to the interior cells' f* (pred_planes.hpp: BUOY)
template <bool SUPG, int NM, bool ZP, typename... M>
__global__ __launch_bounds__(256) void k_predictor3d(const float *__restrict__ u, const float *__restrict__ v,
                                                     const float *__restrict__ w, float nu,
                                                     float *__restrict__ us, float *__restrict__ vs,
                                                     float *__restrict__ ws, float *__restrict__ tau_out, int nz,
                                                     int ny, int nx, float dt, PredK3 kk, M... mode) {
    CFD_3D_INDEX
    if (!cell) return;
    const float uc = u[c], vc = v[c], wc = w[c];
    float uo = uc, vo = vc, wo = wc, t = 0.0f;  // the six faces keep f (tau, nu_t: 0)
    [[maybe_unused]] float nt = 0.0f;
    constexpr bool BUOY = (std::is_same_v<M, Pred3Buoy> || ...);
    static_assert(!BUOY || NM != kNu3Array, "buoyancy: scalar and LES viscosity only");
    [[maybe_unused]] const Pred3Nu m = pred3_mode_nu(mode...);
    if (interior3z<ZP>(k, j, i, nz, ny, nx)) {
        CFD_3D_UD(ZP)
        const Nb7 fu = {uc, u[c + 1], u[c - 1], u[c + sy], u[c - sy], u[cu], u[cd]};
        const Nb7 fv = {vc, v[c + 1], v[c - 1], v[c + sy], v[c - sy], v[cu], v[cd]};
        const Nb7 fw = {wc, w[c + 1], w[c - 1], w[c + sy], w[c - sy], w[cu], w[cd]};
        if constexpr (NM == kNu3Array) nu = m.nu_arr[c];
        if constexpr (NM == kNu3Les) {
            nt = smag3_nut(fu, fv, fw, m.c2, kk);
            nu = (nu + nt) + m.art;
        }
        if (SUPG) t = pred3_tau(uc, vc, wc, nu, dt, kk);
        uo = pred3_cell<SUPG>(uc, vc, wc, fu, t, nu, dt, kk);
        vo = pred3_cell<SUPG>(uc, vc, wc, fv, t, nu, dt, kk);
        wo = pred3_cell<SUPG>(uc, vc, wc, fw, t, nu, dt, kk);
        if constexpr (BUOY) {
            const Pred3Buoy bm = pred3_mode_buoy(mode...);
            const float th = bm.T[c] - bm.t_ref;
            uo = uo + dt * (bm.bx * th);
            vo = vo + dt * (bm.by * th);
            wo = wo + dt * (bm.bz * th);
        }
    }
    us[c] = uo;
    vs[c] = vo;
    ws[c] = wo;
    if (tau_out) tau_out[c] = t;  // zeros without SUPG
    if constexpr (NM == kNu3Les)
        if (m.nut) m.nut[c] = nt;
}

// smag3_nut on the interior, 0 on the six faces
__global__ __launch_bounds__(256) void k_smagorinsky3d(const float *__restrict__ u, const float *__restrict__ v,
                                                       const float *__restrict__ w, float *__restrict__ nut, int nz,
                                                       int ny, int nx, float c2, PredK3 kk) {
    CFD_3D_INDEX
    if (!cell) return;
    float nt = 0.0f;
    if (interior3(k, j, i, nz, ny, nx)) {
        // only C, E, N, U are read
        const Nb7 fu = {u[c], u[c + 1], 0.0f, u[c + sy], 0.0f, u[c + sz], 0.0f};
        const Nb7 fv = {v[c], v[c + 1], 0.0f, v[c + sy], 0.0f, v[c + sz], 0.0f};
        const Nb7 fw = {w[c], w[c + 1], 0.0f, w[c + sy], 0.0f, w[c + sz], 0.0f};
        nt = smag3_nut(fu, fv, fw, c2, kk);
    }
    nut[c] = nt;
}

// ((uE - uW) cx + (vN - vS) cy) + (wU - wD) cz, 0 on the six faces (+ max|div|)
template <bool ZP>
__global__ __launch_bounds__(256) void k_divergence3d(const float *__restrict__ u, const float *__restrict__ v,
                                                      const float *__restrict__ w, float *__restrict__ div, int nz,
                                                      int ny, int nx, float cx, float cy, float cz, float *absmax) {
    CFD_3D_INDEX
    float m = 0.0f;
    if (cell) {
        float d = 0.0f;
        if (interior3z<ZP>(k, j, i, nz, ny, nx)) {
            CFD_3D_UD(ZP)
            d = ((u[c + 1] - u[c - 1]) * cx + (v[c + sy] - v[c - sy]) * cy) + (w[cu] - w[cd]) * cz;
        }
        div[c] = d;
        const float a = fabsf(d);
        if (a > m) m = a;
    }
    if (absmax) wave_reduce_max_store(m, absmax);
}

// gradient of phi (0 on the faces), u = u* - dt gx, v = v* - dt gy,
// w = w* - dt gz; gradmax <- max sqrt((gx^2 + gy^2) + gz^2)
template <bool ZP>
__global__ __launch_bounds__(256) void k_project3d(const float *__restrict__ phi, const float *__restrict__ us,
                                                   const float *__restrict__ vs, const float *__restrict__ ws,
                                                   float *__restrict__ u, float *__restrict__ v,
                                                   float *__restrict__ w, int nz, int ny, int nx, float cx, float cy,
                                                   float cz, float dt, float *gradmax) {
    CFD_3D_INDEX
    float m = 0.0f;
    if (cell) {
        float uo = us[c], vo = vs[c], wo = ws[c];  // the faces copy u* through
        if (interior3z<ZP>(k, j, i, nz, ny, nx)) {
            CFD_3D_UD(ZP)
            const float gx = (phi[c + 1] - phi[c - 1]) * cx;
            const float gy = (phi[c + sy] - phi[c - sy]) * cy;
            const float gz = (phi[cu] - phi[cd]) * cz;
            uo = uo - dt * gx;
            vo = vo - dt * gy;
            wo = wo - dt * gz;
            if (gradmax) {
                const float g = sqrtf((gx * gx + gy * gy) + gz * gz);
                if (g > m) m = g;
            }
        }
        u[c] = uo;
        v[c] = vo;
        w[c] = wo;
    }
    if (gradmax) wave_reduce_max_store(m, gradmax);
}

// Lid-driven cavity walls in 3-D (host_lid_bc's pattern): u = v = w = 0 on the
// six faces, then the face y = ny - 1 gets u = u_lid, v = w = 0; the lid is
// written last, so it owns its edges.  One thread per cell of the largest
// face; a cell on an edge is written by the threads of both its faces with
// the same value (u_lid on row ny - 1, else 0).
__global__ void k_lid_bc3d(float *__restrict__ u, float *__restrict__ v, float *__restrict__ w, int nz, int ny,
                           int nx, float u_lid) {
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t sy = (size_t)nx, sz = (size_t)ny * nx;
    auto put = [&](size_t c, bool lid) {
        u[c] = lid ? u_lid : 0.0f;
        v[c] = 0.0f;
        w[c] = 0.0f;
    };
    if (t < sz) {  // planes z = 0 and z = nz - 1
        const bool lid = t / sy == (size_t)(ny - 1);
        put(t, lid);
        put((size_t)(nz - 1) * sz + t, lid);
    }
    if (t < (size_t)nz * nx) {  // rows y = 0 and y = ny - 1 (the lid)
        const size_t k = t / nx, i = t % nx;
        put(k * sz + i, false);
        put(k * sz + (size_t)(ny - 1) * sy + i, true);
    }
    if (t < (size_t)nz * ny) {  // columns x = 0 and x = nx - 1
        const size_t k = t / ny, j = t % ny;
        const bool lid = j == (size_t)(ny - 1);
        put(k * sz + j * sy, lid);
        put(k * sz + j * sy + (nx - 1), lid);
    }
}

// Channel boundary conditions and the immersed-boundary forcing of the 3-D
// cylinder channel (axis along z), one launch on u, v, w.  Net effect, in this
// order (tests/cyl3d_reference.py states it as NumPy): inlet column x = 0
// (u = k_bc's inlet value of row i, v = w = 0), outlet copy nx-1 <- nx-2,
// free-slip spanwise faces (u, v of planes 0 / nz-1 <- planes 1 / nz-2, w = 0),
// channel walls i = 0 and ny-1 at 0 (written last), then ibm_cell with the 2-D
// float64 mask m[i, j] on every plane.
//
// Ownership: every cell is written by one thread and no thread reads a cell
// another one writes.  The owners are the cells (k, i, j) with 1 <= k <= nz-2
// and j <= nx-2: an owner forms its value after the walls ("before"), applies
// the IBM factor, and also writes the cells that copy from it -- (k, i, nx-1)
// when j == nx-2, and the same cells of plane 0 when k == 1 and of plane nz-1
// when k == nz-2 (nz == 3: both).  A cell (k', i, j') belongs to the owner
// (clamp(k', 1, nz-2), i, min(j', nx-2)).  Only owners with something to write
// are visited, in four disjoint index ranges: planes 1 and nz-2 whole; on the
// planes between them the wall rows, the columns 0 and nx-2, and the box
// [i0, i1) x [j0, j1) of the mask clipped to the cells left over.  The mask is
// read inside the box only (0 elsewhere), so the stage costs its faces plus
// the box and not a pass over the fields.
//
// ZP (cfd_apply_channel_bc_ibm3d_zper_f32, spanwise-periodic): the assignments
// without the face step.  There are no face planes: every plane's cells
// (k, i, j <= nx-2) are owners, a cell (k, i, j') belongs to the owner
// (k, i, min(j', nx-2)), and the visited ranges are the wall rows, the columns
// 0 and nx-2 and the clipped box on all nz planes.
struct BcIbm3 {
    float *u, *v, *w;
    const double *y, *m;
    int nz, ny, nx;
    double y_max, v_inf;
    int step;
    double fs;
    int i0, i1, j0, j1;
    double *force;  // += sum (before - after) of u, v, w over the cells with m > 0
};

template <bool ZP>
__device__ inline void bc_ibm3_own(const BcIbm3 &a, int k, int i, int j, double (&f)[3]) {
    const size_t sy = (size_t)a.nx, sz = (size_t)a.ny * a.nx;
    const size_t c = (size_t)k * sz + (size_t)i * sy + j;
    auto mk = [&](int jj) {
        return a.m && i >= a.i0 && i < a.i1 && jj >= a.j0 && jj < a.j1 ? a.m[(size_t)i * sy + jj] : 0.0;
    };
    const bool wall = i == 0 || i == a.ny - 1, east = j == a.nx - 2;
    const bool keep = !wall && j != 0;  // the assignments leave the owner's own value
    const double mv = mk(j), me = east ? mk(a.nx - 1) : 0.0;
    if (keep && !east && (ZP || (k != 1 && k != a.nz - 2)) && !(mv > 0.0)) return;  // nothing to write
    float b[3] = {0.0f, 0.0f, 0.0f};
    if (keep) {
        b[0] = a.u[c];
        b[1] = a.v[c];
        b[2] = a.w[c];
    } else if (!wall) {  // the inlet, as k_bc forms it
        const double s = (double)a.step;
        double scale = s / 1000.0;
        scale = (1.0 < scale ? 1.0 : scale) * 0.01;
        const double two_pi = 2.0 * 3.141592653589793;
        const double pert = scale * sin(two_pi * a.y[i] / a.y_max + 0.02 * s);
        b[0] = (float)(a.v_inf * (1.0 + pert));
    }
    float *const fld[3] = {a.u, a.v, a.w};
    // one cell: its value before the IBM factor is b (w: 0 on a spanwise face)
    auto put = [&](size_t cc, double mm, bool face, bool same) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float before = q == 2 && face ? 0.0f : b[q];
            const float after = ibm_cell(before, mm, a.fs);
            if (!same || mm > 0.0) fld[q][cc] = after;
            if (mm > 0.0) f[q] += (double)before - (double)after;
        }
    };
    put(c, mv, false, keep);
    if (east) put(c + 1, me, false, false);
    if constexpr (ZP) return;
    if (k == 1) {
        put(c - sz, mv, true, false);
        if (east) put(c - sz + 1, me, true, false);
    }
    if (k == a.nz - 2) {
        put(c + sz, mv, true, false);
        if (east) put(c + sz + 1, me, true, false);
    }
}

template <bool ZP>
__global__ __launch_bounds__(256) void k_channel_bc_ibm3d(BcIbm3 a, size_t n_plane, size_t n_rows, size_t n_cols,
                                                          size_t n_box, int bi0, int bj0, int bh, int bw) {
    __shared__ double part[4][3];
    double f[3] = {0.0, 0.0, 0.0};
    const size_t total = n_plane + n_rows + n_cols + n_box;
    const size_t ex = (size_t)(a.nx - 1);  // owners of a row
    constexpr int KB = ZP ? 0 : 2;         // first plane of the three ranges after n_plane (ZP: n_plane = 0)
    for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
        size_t r = t;
        if (r < n_plane) {  // planes 1 and nz - 2
            const int i = (int)(r / ex), j = (int)(r % ex);
            bc_ibm3_own<ZP>(a, 1, i, j, f);
            if (a.nz > 3) bc_ibm3_own<ZP>(a, a.nz - 2, i, j, f);
            continue;
        }
        r -= n_plane;
        if (r < n_rows) {  // the wall rows of planes 2 .. nz - 3
            const int k = KB + (int)(r / (2 * ex));
            const size_t q = r % (2 * ex);
            bc_ibm3_own<ZP>(a, k, q < ex ? 0 : a.ny - 1, (int)(q % ex), f);
            continue;
        }
        r -= n_rows;
        if (r < n_cols) {  // columns 0 and nx - 2 of rows 1 .. ny - 2 of those planes
            const size_t per = 2 * (size_t)(a.ny - 2);
            const int k = KB + (int)(r / per);
            const size_t q = r % per;
            bc_ibm3_own<ZP>(a, k, 1 + (int)(q >> 1), (q & 1) ? a.nx - 2 : 0, f);
            continue;
        }
        r -= n_cols;  // the rest of the mask's box on those planes
        const size_t per = (size_t)bh * bw;
        const size_t q = r % per;
        bc_ibm3_own<ZP>(a, KB + (int)(r / per), bi0 + (int)(q / bw), bj0 + (int)(q % bw), f);
    }
    if (!a.force) return;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) f[q] += __shfl_xor(f[q], off, kWave);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][q] = f[q];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int q = threadIdx.x;
        const double s = ((part[0][q] + part[1][q]) + part[2][q]) + part[3][q];
        if (s != 0.0) atomicAdd(a.force + q, s);  // a NaN is added too
    }
}

// The vorticity vector of u, v, w from central differences (k_vorticity's
// divisions by f32(2 d)), 0 on the six faces, NaN where mask != 0; mag =
// sqrt((ox ox + oy oy) + oz oz); absmax <- nanmax(mag).  Null outputs are
// not stored.
template <bool ZP>
__global__ __launch_bounds__(256) void k_vorticity3d(const float *__restrict__ u, const float *__restrict__ v,
                                                     const float *__restrict__ w, const uint8_t *__restrict__ mask,
                                                     float *__restrict__ ox, float *__restrict__ oy,
                                                     float *__restrict__ oz, float *__restrict__ mag, float *absmax,
                                                     int nz, int ny, int nx, float dx2, float dy2, float dz2) {
    CFD_3D_INDEX
    float m = 0.0f;
    if (cell) {
        float x = 0.0f, y = 0.0f, z = 0.0f, g = 0.0f;
        if (mask && mask[c]) {
            x = y = z = g = __builtin_nanf("");
        } else if (interior3z<ZP>(k, j, i, nz, ny, nx)) {
            CFD_3D_UD(ZP)
            x = (w[c + sy] - w[c - sy]) / dy2 - (v[cu] - v[cd]) / dz2;
            y = (u[cu] - u[cd]) / dz2 - (w[c + 1] - w[c - 1]) / dx2;
            z = (v[c + 1] - v[c - 1]) / dx2 - (u[c + sy] - u[c - sy]) / dy2;
            g = sqrtf((x * x + y * y) + z * z);
            if (g > m) m = g;  // a NaN never wins
        }
        if (ox) ox[c] = x;
        if (oy) oy[c] = y;
        if (oz) oz[c] = z;
        if (mag) mag[c] = g;
    }
    if (absmax) wave_reduce_max_store(m, absmax);
}

// Mean of 0.5 ((u*u + v*v) + w*w) over n cells, then the three clips, in one
// launch: k_energy_mean_mb's scheme (block b folds a fixed contiguous range
// thread-strided into float64 partials, the last block to take a ticket adds
// the block partials in block order: the same bits run to run) on three
// fields and up to kEnergy3Blocks blocks.  Each cell's energy is formed in
// float32 from the values loaded (before the clip).  The partials and the
// ticket live in a slot of static device memory (no allocation): one slot per
// (device, stream), handed out on the host.
constexpr int kEnergy3Blocks = 512;
constexpr int kEnergy3Slots = 32;
struct Energy3Slot {
    unsigned ticket;  // zero between calls (the last block resets it)
    double partial[kEnergy3Blocks];
};
__device__ Energy3Slot g_energy3[kEnergy3Slots];

__global__ __launch_bounds__(256) void k_energy_mean_clip3d(float *__restrict__ u, float *__restrict__ v,
                                                            float *__restrict__ w, size_t n, double *out, float lo,
                                                            float hi, int slot) {
    constexpr int U = 4;
    __shared__ double part[4];
    __shared__ int last;
    __shared__ double all[kEnergy3Blocks];
    Energy3Slot &ws = g_energy3[slot];
    const size_t per = (n + gridDim.x - 1) / gridDim.x;
    const size_t b0 = blockIdx.x * per < n ? blockIdx.x * per : n, b1 = b0 + per < n ? b0 + per : n;
    double s[U];
#pragma unroll
    for (int q = 0; q < U; ++q) s[q] = 0.0;
    auto cell = [&](size_t c, double &acc) {
        const float a = u[c], b = v[c], d = w[c];
        acc += (double)(0.5f * ((a * a + b * b) + d * d));
        u[c] = clip_val(a, lo, hi);
        v[c] = clip_val(b, lo, hi);
        w[c] = clip_val(d, lo, hi);
    };
    size_t c = b0 + threadIdx.x;
    for (; c + (U - 1) * 256 < b1; c += U * 256) {
#pragma unroll
        for (int q = 0; q < U; ++q) cell(c + q * 256, s[q]);
    }
#pragma unroll
    for (int q = 0; q < U; ++q)
        if (c + q * 256 < b1) cell(c + q * 256, s[q]);
    double t = s[0];
#pragma unroll
    for (int q = 1; q < U; ++q) t += s[q];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, kWave);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        ws.partial[blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
        __threadfence();  // the partial before the ticket
        last = atomicAdd(&ws.ticket, 1u) == (unsigned)gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    for (int q = threadIdx.x; q < (int)gridDim.x; q += blockDim.x)
        all[q] = __hip_atomic_load(&ws.partial[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = 0.0;
        for (int q = 0; q < (int)gridDim.x; ++q) r += all[q];
        *out = r * (1.0 / (double)n);
        __hip_atomic_store(&ws.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the (device, stream)'s slot of g_energy3, or -1 when all are taken
static int energy3_slot(hipStream_t s) {
    static std::mutex mu;
    static std::map<std::pair<int, hipStream_t>, int> slots;
    static int used[64] = {};  // per device
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return -1;
    std::lock_guard<std::mutex> lk(mu);
    auto it = slots.find({dev, s});
    if (it != slots.end()) return it->second;
    if (used[dev] >= kEnergy3Slots) return -1;
    return slots[{dev, s}] = used[dev]++;
}

static dim3 grid3d(int nz, int ny, int nx) { return dim3(ceil_div(nx, 256), ny, nz); }

static thread_local int g_last_pred3[2] = {-1, 0};

}  // namespace cfd

using namespace cfd;

// every dimension >= 3 (one interior cell), rows and planes within a launch grid
#define CFD_SHAPE3D(who, nz, ny, nx)                                                                        \
    CFD_REQUIRE((nz) >= 3 && (ny) >= 3 && (nx) >= 3 && (ny) <= 65535 && (nz) <= 65535,                       \
                "%s: bad 3-D shape (%d, %d, %d): every dimension 3 .. 65535 (nx: any >= 3)", who, nz, ny, nx)

// The entry points of the fused predictor (nm: the viscosity mode).  nu_arr
// (kNu3Array) is an input, nut (kNu3Les, may be null) an output.  buoy: the
// buoyant form (buoyancy3d.hip's entry points; scalar and LES only), null for
// the plain one -- the same dispatch either way.
int cfd::predictor3d_run(const char *who, int nm, bool zper, const float *u, const float *v, const float *w,
                         float nu, const float *nu_arr, float art, double cs, float *u_star, float *v_star,
                         float *w_star, float *tau, float *nut, int nz, int ny, int nx, double dx, double dy,
                         double dz, float dt, int use_supg, void *stream, const Pred3Buoy *buoy) {
    CFD_REQUIRE(u && v && w && u_star && v_star && w_star && (nm != kNu3Array || nu_arr), "%s: null pointer", who);
    CFD_REQUIRE(!buoy || (buoy->T && nm != kNu3Array), "%s: null pointer: T", who);
    CFD_SHAPE3D(who, nz, ny, nx);
    const float *T = buoy ? buoy->T : nullptr;
    const float *in[5] = {u, v, w, nu_arr, T};
    float *out[5] = {u_star, v_star, w_star, tau, nut};
    for (int o = 0; o < 5; ++o) {
        if (!out[o]) continue;
        for (int q = 0; q < 5; ++q) CFD_REQUIRE(out[o] != in[q], "%s: outputs must not alias inputs", who);
        for (int p = 0; p < o; ++p) CFD_REQUIRE(out[o] != out[p], "%s: outputs must not alias each other", who);
    }
    const PredK3 k = make_pred_k3(dx, dy, dz);
    const float c2 = nm == kNu3Les ? (float)smag3_const(cs, dx, dy, dz) : 0.0f;
    hipStream_t s = as_stream(stream);
    // cells per lane of the plane march: the preferred count (tuning; auto: 4,
    // 2 where a 256-column segment would be wider than the grid), halved until
    // nx and every array's alignment allow it (1 always does)
    int vec = tuning().pred3_vec;
    if (!vec) vec = nx < 256 ? 2 : 4;
    auto fits = [&](int c) {
        const uintptr_t m = (uintptr_t)(4 * c - 1);
        auto al = [&](const void *p_) { return !p_ || ((uintptr_t)p_ & m) == 0; };
        return nx % c == 0 && al(u) && al(v) && al(w) && al(u_star) && al(v_star) && al(w_star) && al(tau) &&
               al(nu_arr) && al(nut) && al(T);
    };
    while (vec > 1 && !fits(vec)) vec /= 2;
    // the march runs where a plane's byte offsets fit its buffer resource and
    // (auto) nx and the alignment leave it more than one cell per lane; a
    // forced march (variant 2) also runs at one
    const bool plane_ok = (size_t)ny * nx * sizeof(float) < ((size_t)1 << 31);
    const int variant = tuning().pred3_variant;
    const bool march = plane_ok && variant != 1 && (variant == 2 || vec > 1);
    // LES with SUPG is the one instantiation where arithmetic shows: where the
    // march runs, auto takes it at one cell per lane (the fastest measured
    // shape at 512^3 SUPG); a given cells_per_lane is kept
    if (march && nm == kNu3Les && use_supg && !tuning().pred3_vec) vec = 1;
    const int tk = timing_begin(s, kTimingPredictor);
    if (march) {
        Pred3Args a;
        a.u = u;
        a.v = v;
        a.w = w;
        a.us = u_star;
        a.vs = v_star;
        a.ws = w_star;
        a.tau = tau;
        a.nu = nu;
        a.dt = dt;
        a.nz = nz;
        a.ny = ny;
        a.nx = nx;
        a.k = k;
        a.nu_arr = nu_arr;
        a.nut = nut;
        a.c2 = c2;
        a.art = art;
        a.T = T;
        a.bx = buoy ? buoy->bx : 0.0f;
        a.by = buoy ? buoy->by : 0.0f;
        a.bz = buoy ? buoy->bz : 0.0f;
        a.t_ref = buoy ? buoy->t_ref : 0.0f;
        const int rows = tuning().pred3_rows ? tuning().pred3_rows : 2;
        if (buoy) CFD_CHECK_HIP(pred_planes_launch_buoyant(a, use_supg != 0, nm, vec, rows, s, zper));
        else CFD_CHECK_HIP(pred_planes_launch(a, use_supg != 0, nm, vec, rows, 0, s, zper));
        g_last_pred3[0] = 1;
        g_last_pred3[1] = vec;
    } else {
        const Pred3Nu m = {nu_arr, nut, c2, art};
        const dim3 g = grid3d(nz, ny, nx);
#define CFD_PRED3_CELL(KERNEL, ...)                                                                        \
    hipLaunchKernelGGL(KERNEL, g, dim3(256), 0, s, u, v, w, nu, u_star, v_star, w_star, tau, nz, ny, nx, dt, k, \
                       ##__VA_ARGS__)
        if (buoy && zper && nm == kNu3Les) {
            if (use_supg) CFD_PRED3_CELL((k_predictor3d<true, kNu3Les, true, Pred3Nu, Pred3Buoy>), m, *buoy);
            else CFD_PRED3_CELL((k_predictor3d<false, kNu3Les, true, Pred3Nu, Pred3Buoy>), m, *buoy);
        } else if (buoy && zper) {
            if (use_supg) CFD_PRED3_CELL((k_predictor3d<true, kNu3Scalar, true, Pred3Buoy>), *buoy);
            else CFD_PRED3_CELL((k_predictor3d<false, kNu3Scalar, true, Pred3Buoy>), *buoy);
        } else if (buoy && nm == kNu3Les) {
            if (use_supg) CFD_PRED3_CELL((k_predictor3d<true, kNu3Les, false, Pred3Nu, Pred3Buoy>), m, *buoy);
            else CFD_PRED3_CELL((k_predictor3d<false, kNu3Les, false, Pred3Nu, Pred3Buoy>), m, *buoy);
        } else if (buoy) {
            if (use_supg) CFD_PRED3_CELL((k_predictor3d<true, kNu3Scalar, false, Pred3Buoy>), *buoy);
            else CFD_PRED3_CELL((k_predictor3d<false, kNu3Scalar, false, Pred3Buoy>), *buoy);
        } else if (zper && nm == kNu3Les) {
            if (use_supg) CFD_PRED3_CELL((k_predictor3d<true, kNu3Les, true, Pred3Nu>), m);
            else CFD_PRED3_CELL((k_predictor3d<false, kNu3Les, true, Pred3Nu>), m);
        } else if (zper) {
            if (use_supg) CFD_PRED3_CELL((k_predictor3d<true, kNu3Scalar, true>));
            else CFD_PRED3_CELL((k_predictor3d<false, kNu3Scalar, true>));
        } else if (nm == kNu3Les) {
            if (use_supg) CFD_PRED3_CELL((k_predictor3d<true, kNu3Les, false, Pred3Nu>), m);
            else CFD_PRED3_CELL((k_predictor3d<false, kNu3Les, false, Pred3Nu>), m);
        } else if (nm == kNu3Array) {
            if (use_supg) CFD_PRED3_CELL((k_predictor3d<true, kNu3Array, false, Pred3Nu>), m);
            else CFD_PRED3_CELL((k_predictor3d<false, kNu3Array, false, Pred3Nu>), m);
        } else {
            if (use_supg) CFD_PRED3_CELL((k_predictor3d<true, kNu3Scalar, false>));
            else CFD_PRED3_CELL((k_predictor3d<false, kNu3Scalar, false>));
        }
#undef CFD_PRED3_CELL
        g_last_pred3[0] = 0;
        g_last_pred3[1] = 1;
    }
    timing_end(tk, s, 1);
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

extern "C" {

int cfd_predictor3d_f32(const float *u, const float *v, const float *w, float nu_eff, float *u_star,
                        float *v_star, float *w_star, float *tau, int nz, int ny, int nx, double dx, double dy,
                        double dz, float dt, int use_supg, void *stream) {
    return predictor3d_run("predictor3d", kNu3Scalar, false, u, v, w, nu_eff, nullptr, 0.0f, 0.0, u_star, v_star,
                           w_star, tau, nullptr, nz, ny, nx, dx, dy, dz, dt, use_supg, stream);
}

int cfd_predictor3d_nu_f32(const float *u, const float *v, const float *w, const float *nu_eff, float *u_star,
                           float *v_star, float *w_star, float *tau, int nz, int ny, int nx, double dx, double dy,
                           double dz, float dt, int use_supg, void *stream) {
    return predictor3d_run("predictor3d_nu", kNu3Array, false, u, v, w, 0.0f, nu_eff, 0.0f, 0.0, u_star, v_star,
                           w_star, tau, nullptr, nz, ny, nx, dx, dy, dz, dt, use_supg, stream);
}

int cfd_predictor3d_les_f32(const float *u, const float *v, const float *w, float nu, float art_visc, double cs,
                            float *u_star, float *v_star, float *w_star, float *tau, float *nu_t, int nz, int ny,
                            int nx, double dx, double dy, double dz, float dt, int use_supg, void *stream) {
    return predictor3d_run("predictor3d_les", kNu3Les, false, u, v, w, nu, nullptr, art_visc, cs, u_star, v_star,
                           w_star, tau, nu_t, nz, ny, nx, dx, dy, dz, dt, use_supg, stream);
}

int cfd_predictor3d_zper_f32(const float *u, const float *v, const float *w, float nu_eff, float *u_star,
                             float *v_star, float *w_star, float *tau, int nz, int ny, int nx, double dx, double dy,
                             double dz, float dt, int use_supg, void *stream) {
    return predictor3d_run("predictor3d_zper", kNu3Scalar, true, u, v, w, nu_eff, nullptr, 0.0f, 0.0, u_star, v_star,
                           w_star, tau, nullptr, nz, ny, nx, dx, dy, dz, dt, use_supg, stream);
}

int cfd_predictor3d_les_zper_f32(const float *u, const float *v, const float *w, float nu, float art_visc, double cs,
                                 float *u_star, float *v_star, float *w_star, float *tau, float *nu_t, int nz,
                                 int ny, int nx, double dx, double dy, double dz, float dt, int use_supg,
                                 void *stream) {
    return predictor3d_run("predictor3d_les_zper", kNu3Les, true, u, v, w, nu, nullptr, art_visc, cs, u_star, v_star,
                           w_star, tau, nu_t, nz, ny, nx, dx, dy, dz, dt, use_supg, stream);
}

int cfd_smagorinsky3d_f32(const float *u, const float *v, const float *w, float *nu_t, int nz, int ny, int nx,
                          double dx, double dy, double dz, double cs, void *stream) {
    CFD_REQUIRE(u && v && w && nu_t, "smagorinsky3d: null pointer");
    CFD_REQUIRE(nu_t != u && nu_t != v && nu_t != w, "smagorinsky3d: nu_t must not alias an input");
    CFD_SHAPE3D("smagorinsky3d", nz, ny, nx);
    hipLaunchKernelGGL(k_smagorinsky3d, grid3d(nz, ny, nx), dim3(256), 0, as_stream(stream), u, v, w, nu_t, nz, ny, nx,
                       (float)smag3_const(cs, dx, dy, dz), make_pred_k3(dx, dy, dz));
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

int cfd_set_predictor3d_config(int variant, int rows, int cells_per_lane) {
    CFD_REQUIRE(variant >= 0 && variant <= 2, "predictor3d config: variant 0 (auto), 1 (per cell) or 2 (plane march)");
    CFD_REQUIRE(rows == 0 || rows == 1 || rows == 2, "predictor3d config: rows per wave 0 (auto), 1 or 2");
    CFD_REQUIRE(cells_per_lane == 0 || cells_per_lane == 1 || cells_per_lane == 2 || cells_per_lane == 4,
                "predictor3d config: cells per lane 0 (auto), 1, 2 or 4");
    tuning().pred3_variant = variant;
    tuning().pred3_rows = rows;
    tuning().pred3_vec = cells_per_lane;
    return CFD_OK;
}

int cfd_get_last_predictor3d_path(int *cells_per_lane) {
    if (cells_per_lane) *cells_per_lane = g_last_pred3[1];
    return g_last_pred3[0];
}

static int divergence3d_run(const char *who, bool zper, const float *u, const float *v, const float *w, float *div,
                            int nz, int ny, int nx, double dx, double dy, double dz, float *absmax, void *stream) {
    CFD_REQUIRE(u && v && w && div, "%s: null pointer", who);
    CFD_REQUIRE(div != u && div != v && div != w, "%s: div must not alias an input", who);
    CFD_SHAPE3D(who, nz, ny, nx);
    const float cx = (float)(0.5 / dx), cy = (float)(0.5 / dy), cz = (float)(0.5 / dz);
    if (zper)
        hipLaunchKernelGGL(k_divergence3d<true>, grid3d(nz, ny, nx), dim3(256), 0, as_stream(stream), u, v, w, div, nz,
                           ny, nx, cx, cy, cz, absmax);
    else
        hipLaunchKernelGGL(k_divergence3d<false>, grid3d(nz, ny, nx), dim3(256), 0, as_stream(stream), u, v, w, div,
                           nz, ny, nx, cx, cy, cz, absmax);
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

int cfd_divergence3d_f32(const float *u, const float *v, const float *w, float *div, int nz, int ny, int nx,
                         double dx, double dy, double dz, float *absmax, void *stream) {
    return divergence3d_run("divergence3d", false, u, v, w, div, nz, ny, nx, dx, dy, dz, absmax, stream);
}

int cfd_divergence3d_zper_f32(const float *u, const float *v, const float *w, float *div, int nz, int ny, int nx,
                              double dx, double dy, double dz, float *absmax, void *stream) {
    return divergence3d_run("divergence3d_zper", true, u, v, w, div, nz, ny, nx, dx, dy, dz, absmax, stream);
}

static int project3d_run(const char *who, bool zper, const float *phi, const float *u_star, const float *v_star,
                         const float *w_star, float *u, float *v, float *w, int nz, int ny, int nx, double dx,
                         double dy, double dz, float dt, float *gradmax, void *stream) {
    CFD_REQUIRE(phi && u_star && v_star && w_star && u && v && w, "%s: null pointer", who);
    const float *in[4] = {phi, u_star, v_star, w_star};
    float *out[3] = {u, v, w};
    for (int o = 0; o < 3; ++o) {
        for (int q = 0; q < 4; ++q) CFD_REQUIRE(out[o] != in[q], "%s: outputs must not alias inputs", who);
        for (int p = 0; p < o; ++p) CFD_REQUIRE(out[o] != out[p], "%s: outputs must not alias each other", who);
    }
    CFD_SHAPE3D(who, nz, ny, nx);
    const float cx = (float)(0.5 / dx), cy = (float)(0.5 / dy), cz = (float)(0.5 / dz);
    if (zper)
        hipLaunchKernelGGL(k_project3d<true>, grid3d(nz, ny, nx), dim3(256), 0, as_stream(stream), phi, u_star, v_star,
                           w_star, u, v, w, nz, ny, nx, cx, cy, cz, dt, gradmax);
    else
        hipLaunchKernelGGL(k_project3d<false>, grid3d(nz, ny, nx), dim3(256), 0, as_stream(stream), phi, u_star,
                           v_star, w_star, u, v, w, nz, ny, nx, cx, cy, cz, dt, gradmax);
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

int cfd_project3d_f32(const float *phi, const float *u_star, const float *v_star, const float *w_star, float *u,
                      float *v, float *w, int nz, int ny, int nx, double dx, double dy, double dz, float dt,
                      float *gradmax, void *stream) {
    return project3d_run("project3d", false, phi, u_star, v_star, w_star, u, v, w, nz, ny, nx, dx, dy, dz, dt, gradmax,
                         stream);
}

int cfd_project3d_zper_f32(const float *phi, const float *u_star, const float *v_star, const float *w_star, float *u,
                           float *v, float *w, int nz, int ny, int nx, double dx, double dy, double dz, float dt,
                           float *gradmax, void *stream) {
    return project3d_run("project3d_zper", true, phi, u_star, v_star, w_star, u, v, w, nz, ny, nx, dx, dy, dz, dt,
                         gradmax, stream);
}

int cfd_apply_lid_bc3d_f32(float *u, float *v, float *w, int nz, int ny, int nx, float u_lid, void *stream) {
    CFD_REQUIRE(u && v && w, "apply_lid_bc3d: null pointer");
    CFD_REQUIRE(u != v && u != w && v != w, "apply_lid_bc3d: u, v, w must be three arrays");
    CFD_SHAPE3D("apply_lid_bc3d", nz, ny, nx);
    size_t n = (size_t)ny * nx;
    if ((size_t)nz * nx > n) n = (size_t)nz * nx;
    if ((size_t)nz * ny > n) n = (size_t)nz * ny;
    hipLaunchKernelGGL(k_lid_bc3d, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), u, v, w, nz,
                       ny, nx, u_lid);
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

int cfd_energy_mean_clip3d_f32(float *u, float *v, float *w, size_t n, double *out, float lo, float hi,
                               void *stream) {
    CFD_REQUIRE(u && v && w && out && n > 0, "energy_mean_clip3d_f32: bad arguments");
    CFD_REQUIRE(u != v && u != w && v != w, "energy_mean_clip3d_f32: u, v, w must be three arrays");
    hipStream_t s = as_stream(stream);
    const int slot = energy3_slot(s);
    CFD_REQUIRE(slot >= 0, "energy_mean_clip3d_f32: more than %d streams of one device in use", kEnergy3Slots);
    size_t nb = (n + 4095) / 4096;  // ~16 cells per thread
    if (nb > (size_t)kEnergy3Blocks) nb = kEnergy3Blocks;
    hipLaunchKernelGGL(k_energy_mean_clip3d, dim3((unsigned)nb), dim3(256), 0, s, u, v, w, n, out, lo, hi, slot);
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

// cfd_apply_channel_bc_ibm3d_f32 and, zper, cfd_apply_channel_bc_ibm3d_zper_f32
static int channel_bc_ibm3d_run(const char *who, bool zper, float *u, float *v, float *w, const double *y,
                                const double *ibm_mask2d, int nz, int ny, int nx, double y_max, double v_inf,
                                int step, double force_strength, int i0, int i1, int j0, int j1, double *force_out,
                                void *stream) {
    CFD_REQUIRE(u && v && w && y, "%s: null pointer", who);
    CFD_REQUIRE(u != v && u != w && v != w, "%s: u, v, w must be three arrays", who);
    CFD_SHAPE3D(who, nz, ny, nx);
    CFD_REQUIRE(i0 >= 0 && i0 <= i1 && i1 <= ny && j0 >= 0 && j0 <= j1 && j1 <= nx,
                "%s: box [%d, %d) x [%d, %d) outside the (%d, %d) plane", who, i0, i1, j0, j1, ny, nx);
    CFD_REQUIRE(!ibm_mask2d || (i0 < i1 && j0 < j1), "%s: empty box [%d, %d) x [%d, %d) with a mask", who, i0, i1,
                j0, j1);
    BcIbm3 a;
    a.u = u;
    a.v = v;
    a.w = w;
    a.y = y;
    a.m = ibm_mask2d;
    a.nz = nz;
    a.ny = ny;
    a.nx = nx;
    a.y_max = y_max;
    a.v_inf = v_inf;
    a.step = step;
    a.fs = force_strength;
    a.i0 = i0;
    a.i1 = i1;
    a.j0 = j0;
    a.j1 = j1;
    a.force = force_out;
    // the four ranges of owners (k_channel_bc_ibm3d); periodic: no face planes, the other three on all planes
    const size_t mid = zper ? (size_t)nz : (nz > 4 ? (size_t)(nz - 4) : 0), ex = (size_t)(nx - 1);
    const int bi0 = i0 > 1 ? i0 : 1, bi1 = i1 < ny - 1 ? i1 : ny - 1;
    const int bj0 = j0 > 1 ? j0 : 1, bj1 = j1 < nx - 2 ? j1 : nx - 2;
    const int bh = bi1 > bi0 ? bi1 - bi0 : 0, bw = bj1 > bj0 ? bj1 - bj0 : 0;
    const size_t n_plane = zper ? 0 : (size_t)ny * ex, n_rows = mid * 2 * ex, n_cols = mid * 2 * (size_t)(ny - 2);
    const size_t n_box = ibm_mask2d ? mid * (size_t)bh * bw : 0;
    size_t blocks = (n_plane + n_rows + n_cols + n_box + 255) / 256;
    if (blocks > ((size_t)1 << 20)) blocks = (size_t)1 << 20;  // the kernel strides
    if (zper)
        hipLaunchKernelGGL(k_channel_bc_ibm3d<true>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), a,
                           n_plane, n_rows, n_cols, n_box, bi0, bj0, bh, bw);
    else
        hipLaunchKernelGGL(k_channel_bc_ibm3d<false>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), a,
                           n_plane, n_rows, n_cols, n_box, bi0, bj0, bh, bw);
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

int cfd_apply_channel_bc_ibm3d_f32(float *u, float *v, float *w, const double *y, const double *ibm_mask2d, int nz,
                                   int ny, int nx, double y_max, double v_inf, int step, double force_strength,
                                   int i0, int i1, int j0, int j1, double *force_out, void *stream) {
    return channel_bc_ibm3d_run("apply_channel_bc_ibm3d", false, u, v, w, y, ibm_mask2d, nz, ny, nx, y_max, v_inf,
                                step, force_strength, i0, i1, j0, j1, force_out, stream);
}

int cfd_apply_channel_bc_ibm3d_zper_f32(float *u, float *v, float *w, const double *y, const double *ibm_mask2d,
                                        int nz, int ny, int nx, double y_max, double v_inf, int step,
                                        double force_strength, int i0, int i1, int j0, int j1, double *force_out,
                                        void *stream) {
    return channel_bc_ibm3d_run("apply_channel_bc_ibm3d_zper", true, u, v, w, y, ibm_mask2d, nz, ny, nx, y_max,
                                v_inf, step, force_strength, i0, i1, j0, j1, force_out, stream);
}

static int vorticity3d_run(const char *who, bool zper, const float *u, const float *v, const float *w,
                           const uint8_t *mask, float *ox, float *oy, float *oz, float *mag, float *absmax, int nz,
                           int ny, int nx, double dx, double dy, double dz, void *stream) {
    CFD_REQUIRE(u && v && w, "%s: null pointer", who);
    CFD_REQUIRE(ox || oy || oz || mag || absmax, "%s: no output given", who);
    float *out[4] = {ox, oy, oz, mag};
    for (int o = 0; o < 4; ++o) {
        if (!out[o]) continue;
        CFD_REQUIRE(out[o] != u && out[o] != v && out[o] != w, "%s: outputs must not alias inputs", who);
        for (int p = 0; p < o; ++p) CFD_REQUIRE(out[o] != out[p], "%s: outputs must not alias each other", who);
    }
    CFD_SHAPE3D(who, nz, ny, nx);
    const float dx2 = (float)(2.0 * dx), dy2 = (float)(2.0 * dy), dz2 = (float)(2.0 * dz);
    if (zper)
        hipLaunchKernelGGL(k_vorticity3d<true>, grid3d(nz, ny, nx), dim3(256), 0, as_stream(stream), u, v, w, mask, ox,
                           oy, oz, mag, absmax, nz, ny, nx, dx2, dy2, dz2);
    else
        hipLaunchKernelGGL(k_vorticity3d<false>, grid3d(nz, ny, nx), dim3(256), 0, as_stream(stream), u, v, w, mask, ox,
                           oy, oz, mag, absmax, nz, ny, nx, dx2, dy2, dz2);
    CFD_LAUNCH_CHECK();
    return CFD_OK;
}

int cfd_vorticity3d_f32(const float *u, const float *v, const float *w, const uint8_t *mask, float *ox, float *oy,
                        float *oz, float *mag, float *absmax, int nz, int ny, int nx, double dx, double dy, double dz,
                        void *stream) {
    return vorticity3d_run("vorticity3d", false, u, v, w, mask, ox, oy, oz, mag, absmax, nz, ny, nx, dx, dy, dz,
                           stream);
}

int cfd_vorticity3d_zper_f32(const float *u, const float *v, const float *w, const uint8_t *mask, float *ox,
                             float *oy, float *oz, float *mag, float *absmax, int nz, int ny, int nx, double dx,
                             double dy, double dz, void *stream) {
    return vorticity3d_run("vorticity3d_zper", true, u, v, w, mask, ox, oy, oz, mag, absmax, nz, ny, nx, dx, dy, dz,
                           stream);
}

}  // extern "C"
